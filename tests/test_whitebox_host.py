"""The white-box surface without a GPU: the two entry points and the two hooks are declared in the headers and exported by
the built library; Engine's and PGD's signatures; PGD's marshalling and checkpoint layout on a stub engine; attack_main's
--attack pgd rules with stub models as tests/test_driver_rules.py uses them."""
import contextlib
import ctypes as C
import inspect
import io
import os
import pickle
import re

import numpy as np
import pytest

from fakebob_amd import _native as N
from fakebob_amd import attack_main as AM
from fakebob_amd.attack import FakeBob
from fakebob_amd.engine import Engine
from fakebob_amd.pgd import PGD
from tests.golden import driver_site as DS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header(name):
    with open(os.path.join(ROOT, "include", name)) as r:
        return r.read()


def test_entry_points_are_declared_and_exported():
    pub, hooks = _header("fakebob_hip.h"), _header("fakebob_hip_test.h")
    assert re.search(r"int fb_get_grad_wb\(fb_engine \*e, const fb_nes_params \*p, const double \*audio, int64_t N,", pub)
    assert re.search(r"int fb_attack_wb\(fb_engine \*e, const fb_nes_params \*p, const double \*audio, int64_t N, int16_t \*adv_i16,", pub)
    assert re.search(r"int fb_debug_gmm_feat_grad\(fb_engine \*e, const float \*feats, int Tv, const double \*w, double \*out\);", hooks)
    assert re.search(r"int fb_debug_frontend_vjp\(fb_engine \*e, const int16_t \*wav, int64_t n, const double \*cot,", hooks)
    for word in ("FAKEBOB.py:223-299", "straight-through", "first maximum", "FB_E_STATE", "i-vector", "fb_set_eot", "companions",
                 "input-transform", "air channel", "codec", "feature compression", "dither", "BPDA"):
        assert word in pub, word
    lib = C.CDLL(N.LIB_PATH)
    for name in ("fb_get_grad_wb", "fb_attack_wb", "fb_debug_gmm_feat_grad", "fb_debug_frontend_vjp"):
        assert name in N.EXPORTS
        getattr(lib, name)


def test_engine_and_pgd_signatures():
    assert list(inspect.signature(Engine.get_grad_wb).parameters) == ["self", "params", "audio", "want_grad"]
    assert list(inspect.signature(Engine.attack_wb).parameters) == ["self", "params", "audio"]
    assert list(inspect.signature(Engine.debug_gmm_feat_grad).parameters) == ["self", "feats", "w"]
    assert list(inspect.signature(Engine.debug_frontend_vjp).parameters) == ["self", "wav", "cot"]
    fb, pg = inspect.signature(FakeBob.__init__).parameters, inspect.signature(PGD.__init__).parameters
    nes_only = {"samples_per_draw", "sigma", "eot_size"}
    assert [k for k in fb if k not in nes_only] == list(pg)           # FakeBob's knobs minus the NES ones, same order
    for k in pg:
        assert pg[k].default == fb[k].default, k
    fa, pa = inspect.signature(FakeBob.attack).parameters, inspect.signature(PGD.attack).parameters
    assert [k for k in fa if k not in ("noise_all", "companions")] == list(pa)
    for k in pa:
        assert pa[k].default == fa[k].default, k


class _Engine(object):
    kind = "gmm"

    def __init__(self, S):
        self.n_speakers, self.calls = S, []

    def attack_wb(self, p, audio):
        self.calls.append(("wb", p.samples_per_draw, p.max_iter, p.epsilon, p.max_lr, p.min_lr, p.momentum, p.plateau_length,
                           p.plateau_drop, p.threshold, p.target, p.true_label, p.adver_thresh, p.bits_per_sample))
        S = max(self.n_speakers, 1)
        trace = np.arange(3 * (3 + S), dtype=np.float64).reshape(3, 3 + S)
        trace[-1, 1] = -1.0                              # the early-stop row
        return np.arange(audio.size, dtype=np.int16), 1, audio.copy(), trace

    def get_grad_wb(self, p, audio):
        self.calls.append(("grad", p.bits_per_sample))
        return np.ones(audio.size), 0.5, np.arange(max(self.n_speakers, 1), dtype=np.float64)

    def attack_iter_seconds(self, n):
        return 0.25 * (1 + np.arange(n))


class _Model(object):
    def __init__(self, task, S):
        self.task, self.engine = task, _Engine(S)


@pytest.mark.parametrize("task,S", [("OSI", 3), ("SV", 1)])
def test_pgd_marshals_and_writes_fakebobs_checkpoint(tmp_path, task, S):
    m = _Model(task, S)
    pg = PGD(task, "targeted", m, adver_thresh=0.5, epsilon=0.003, max_iter=9, max_lr=2e-3, min_lr=1e-5, momentum=0.0,
             plateau_length=4, plateau_drop=3.0, verbose=False)
    audio = np.linspace(-0.5, 0.5, 40)
    cp = str(tmp_path / "a.cp")
    adv, flag = pg.attack(audio, cp, threshold=0.25, target=2 if task == "OSI" else None, bits_per_sample=12)
    assert adv.dtype == np.int16 and adv.shape == (40, 1) and flag == 1
    assert m.engine.calls == [("wb", 0, 9, 0.003, 2e-3, 1e-5, 0.0, 4, 3.0, 0.25, 2 if task == "OSI" else 0, 0, 0.5, 12)]
    with open(cp, "rb") as r:
        rows = pickle.load(r)
    assert len(rows) == 3
    for k, row in enumerate(rows):                       # FakeBob's layout: [distance, array([adver_loss]), score, used_time]
        assert len(row) == 4 and row[0] == k * (3 + S)
        assert isinstance(row[1], np.ndarray) and row[1].shape == (1,)
        if task == "SV":
            assert np.ndim(row[2]) == 0 and row[2] == k * (3 + S) + 3
        else:
            assert row[2].shape == (S,) and row[2][0] == k * (3 + S) + 3
    assert [row[3] for row in rows] == [0.25, 0.5, 0.0]  # the early-stop row stores 0. (FAKEBOB.py:187)
    adv2, _ = pg.attack(audio[:, None], None)            # a column, no checkpoint
    assert adv2.shape == (40, 1)
    g, al, sc = pg.get_grad(audio, bits_per_sample=8)
    assert g.shape == (40, 1) and al.shape == (1,) and m.engine.calls[-1] == ("grad", 8)
    assert np.ndim(sc) == 0 if task == "SV" else sc.shape == (S,)
    with pytest.raises(ValueError):
        pg.attack(audio, None, bits_per_sample=17)


def test_pgd_refuses_what_it_cannot_differentiate():
    with pytest.raises(ValueError):
        PGD("XYZ", "targeted", _Model("OSI", 3))
    with pytest.raises(ValueError):
        PGD("SV", "targeted", _Model("OSI", 3))          # the model's task
    with pytest.raises(TypeError):
        PGD("OSI", "targeted", object())                 # a foreign model: no engine, no gradient
    iv = _Model("OSI", 3)
    iv.engine.kind = "iv"
    with pytest.raises(ValueError):
        PGD("OSI", "targeted", iv)
    assert "no threshold sweep of its own" in PGD.estimate_threshold.__doc__


# ------------------------------------------------------------------------------------------------ attack_main
@pytest.fixture()
def site(tmp_path):
    DS.make_site(str(tmp_path))
    old = os.getcwd()
    os.chdir(str(tmp_path))
    yield str(tmp_path)
    os.chdir(old)


def _main(extra, built=None):
    seen = []

    def bob(task, at, model, **hp):
        seen.append(hp)
        return DS.StubBob(task, at, model, **hp)

    def model(archi, t, ml, pre, th, gid):
        if built is not None:
            built.append(gid)
        return DS.StubModel(t, th)
    DS.StubBob.log = []
    argv = ["-spk_id"] + DS.SPK_IDS + ["-task", "OSI", "-type", "targeted", "--streams", "1", "--seed", "5"] + extra
    with contextlib.redirect_stdout(io.StringIO()), contextlib.redirect_stderr(io.StringIO()):
        res = AM.main(argv, model_factory=model, bob_factory=bob)
    return res, seen


def test_attack_main_hands_pgd_its_options(site):
    (g, results, _thr), seen = _main(["--attack", "pgd", "-epsilon", "0.004", "-max_iter", "40", "-adver", "0.5", "-momentum", "0",
                                      "-max_lr", "0.002", "-samples", "10", "--eot-size", "1", "--codec", "none"])
    assert seen == [dict(adver_thresh=0.5, epsilon=0.004, max_iter=40, max_lr=0.002, min_lr=1e-6, momentum=0.0, plateau_length=5,
                         plateau_drop=2.0)]                            # no samples_per_draw, no sigma
    assert g[1] == len(results) > 0
    for extra in ([], ["--attack", "nes"]):                            # the default: nothing changes
        _res, seen = _main(extra)
        assert sorted(seen[0]) == sorted(["adver_thresh", "epsilon", "max_iter", "max_lr", "min_lr", "samples_per_draw", "sigma",
                                          "momentum", "plateau_length", "plateau_drop"])


@pytest.mark.parametrize("extra", [["--eot-size", "2"], ["--companions", "1"], ["--input-transform", "ms:7"], ["--air-channel", "t60:200-600"],
                                   ["--codec", "ulaw"], ["--feco", "0.5"], ["--dither", "1.0"], ["-archi", "iv"]])
def test_attack_main_refuses_pgd_before_any_model_is_built(site, extra):
    built = []
    with pytest.raises(SystemExit):
        _main(["--attack", "pgd"] + extra, built)
    assert built == []
