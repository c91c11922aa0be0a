"""CW2 without a GPU: the host twin of fb_attack_cw2 (tests/cw2_ref.py) against torch.optim.Adam, math.fsum and hand-written
search sequences; the surface (header, exports, struct, signatures); CW2's parameter checks and marshalling on a stub engine;
attack_main's --attack cw2 rules with stub models as tests/test_driver_rules.py uses them.

One comparison carries a tolerance: five Adam steps of the twin against torch.optim.Adam on autograd's float64 gradient of
c gate <g, x> + |x - a0|^2, x = tanh(w0 + mod), N = 257.  The two differ in float64 rounding only (autograd forms
1 - tanh^2 and the products in another order, and its tanh need not be numpy's to the last bit).  Measured on the CPU, worst
over the five steps of mod and x, relative to their largest element: 3.38e-15 with the gate open and 8.57e-11 with it closed --
there the only gradient is 2 (x - a0) at x = tanh(atanh(0.999999 a0)), a difference of 1e-6 |a0| between numbers of size
|a0|, which magnifies one ulp of tanh by a million.  ADAM[gate] = (measured, bar); each bar is four times the measured figure.
"""
import contextlib
import ctypes as C
import inspect
import io
import math
import os
import pickle
import re

import numpy as np
import pytest

from fakebob_amd import _native as N
from fakebob_amd import attack_main as AM
from fakebob_amd.cw2 import CW2, check_cw2_params, snr_db
from fakebob_amd.engine import Engine, cw2_params
from fakebob_amd.pgd import PGD
from tests import cw2_ref as R
from tests.golden import driver_site as DS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ADAM = {1: (3.38e-15, 1.4e-14), 0: (8.57e-11, 3.5e-10)}


# ------------------------------------------------------------------------------------------------ the twin
@pytest.mark.parametrize("gate", [0, 1])
def test_adam_step_of_the_twin_is_torch_optim_adam(gate):
    import torch
    n, c, lr = 257, 0.75, 1e-2
    rng = np.random.default_rng(11 + gate)
    a0 = rng.uniform(-0.9, 0.9, n)
    g = rng.normal(size=n)
    w0 = R.w0_of(a0)
    mod_t = torch.zeros(n, dtype=torch.float64, requires_grad=True)
    opt = torch.optim.Adam([mod_t], lr=lr)
    tw0, ta0, tg = torch.from_numpy(w0), torch.from_numpy(a0), torch.from_numpy(g)
    mod, m1, m2, x = np.zeros(n), np.zeros(n), np.zeros(n), np.tanh(w0)
    p1 = p2 = 1.0
    worst = 0.0
    for _step in range(5):
        opt.zero_grad()
        xt = torch.tanh(tw0 + mod_t)
        loss = (c * gate) * torch.dot(tg, xt) + torch.sum((xt - ta0) ** 2)
        loss.backward()
        opt.step()
        p1 *= 0.9
        p2 *= 0.999
        mod, m1, m2, x = R.adam_step(g, x, a0, w0, mod, m1, m2, c, gate, p1, p2, lr=lr)
        ref = mod_t.detach().numpy()
        worst = max(worst, float(np.abs(mod - ref).max() / np.abs(ref).max()),
                    float(np.abs(x - np.tanh(w0 + ref)).max() / np.abs(x).max()))
    print("twin against torch.optim.Adam, gate %d: worst relative difference %.3g" % (gate, worst))
    assert np.abs(mod).max() > 1e-3       # steps of the order of lr: the comparison is not of zeros
    assert worst <= ADAM[gate][1]


@pytest.mark.parametrize("n", [1, 255, 256, 257, 4000])
def test_block_ordered_l2_is_fsum(n):
    rng = np.random.default_rng(n)
    a0 = rng.uniform(-1, 1, n)
    x = a0 + rng.normal(scale=1e-3, size=n)
    want = math.fsum(float(v) * float(v) for v in (x - a0))
    got = R.l2_blocks(x, a0)
    assert abs(got - want) <= 1e-15 * want
    assert R.l2_blocks(a0, a0) == 0.0


def test_block_order_is_the_written_one():
    """terms chosen so that the order shows: a large lane 0 absorbs single ones but not their pairwise sums"""
    d = np.ones(257)
    d[0] = 2.0 ** 30
    x = np.sqrt(d)          # exact roots: the squares are d again
    assert np.array_equal(x * x, d)
    assert R.l2_blocks(x, np.zeros(257)) == 2.0 ** 30 + 255.0 + 1.0
    big = np.zeros(512)
    big[0], big[1], big[129], big[65], big[193] = 2.0 ** 54, 1.0, 1.0, 1.0, 1.0
    assert np.array_equal(np.sqrt(big) ** 2, big)
    # h = 128 pairs lanes 1 + 129 and 65 + 193 -> 2 each; h = 64 brings them together in lane 1 -> 4; h = 1 adds it to lane 0,
    # and 2^54 + 4 is exact, where added one at a time every 1 would be lost
    assert R.l2_blocks(np.sqrt(big), np.zeros(512)) == 2.0 ** 54 + 4.0
    assert (((2.0 ** 54 + 1.0) + 1.0) + 1.0) + 1.0 == 2.0 ** 54


def test_search_constant_rule():
    never, last = R.const_sequence(1e-3, [False] * 9)
    assert never[0] == 1e-3 and all(never[i] == never[i - 1] * 10.0 for i in range(1, 9))  # SpeakerGuard's 1e-3, 1e-2, ...
    assert np.allclose(never, [10.0 ** (k - 3) for k in range(9)], rtol=1e-12) and np.isclose(last, 1e6)
    always, last = R.const_sequence(1e-3, [True] * 5)
    assert always == [1e-3, 5e-4, 2.5e-4, 1.25e-4, 6.25e-5] and last == 3.125e-5            # bisection towards lo = 0
    alt, last = R.const_sequence(1.0, [False, True, False, True])
    # 1 fails -> 10; 10 succeeds: hi = 10, (1 + 10) / 2; 5.5 fails: lo = 5.5, 7.75; succeeds: hi = 7.75 -> 6.625
    assert alt == [1.0, 10.0, 5.5, 7.75] and last == 6.625
    lo, hi, c = R.next_const(False, 0.0, 1e10, 2e8)
    assert (lo, hi, c) == (2e8, 1e10, 2e9)                                                  # tenfold while no success bounds it


def test_control_decisions():
    d = R.control(0.5, 2.0, 3.0, float("inf"), 0, float("inf"), 4)
    assert d["gate"] == 1 and d["take"] == 0 and not d["found"] and not d["abort"] and d["L"] == 3.5 and d["prev"] == 3.5
    d = R.control(-0.5, 2.0, 3.0, float("inf"), 1, 3.5, 4)
    assert d["gate"] == 0 and d["take"] == 1 and d["found"] and d["gbest_l2"] == 2.0 and d["L"] == 2.0 and d["prev"] == 3.5
    assert R.control(-0.5, 2.0, 3.0, 1.5, 1, 3.5, 4)["take"] == 0                           # not smaller than the best
    assert R.control(0.0, 2.0, 3.0, 9.0, 1, 3.5, 4)["take"] == 0 and R.control(0.0, 2.0, 3.0, 9.0, 1, 3.5, 4)["gate"] == 0  # the tie
    assert R.control(0.5, 2.0, 3.0, 9.0, 4, 3.5, 4)["abort"] and not R.control(0.5, 2.0, 3.0, 9.0, 4, 3.5, 0)["abort"]
    assert not R.control(0.5, 2.0, 3.0, 9.0, 5, 3.5, 4)["abort"]                            # not a multiple of abort_every
    assert not R.control(0.5, 1.9, 3.0, 9.0, 4, 3.5, 4)["abort"]                            # fell by more than 0.01 %


# ------------------------------------------------------------------------------------------------ the surface
def test_entry_points_are_declared_and_exported():
    with open(os.path.join(ROOT, "include", "fakebob_hip.h")) as r:
        pub = r.read()
    with open(os.path.join(ROOT, "include", "fakebob_hip_test.h")) as r:
        hooks = r.read()
    assert re.search(r"int fb_attack_cw2\(fb_engine \*e, const fb_nes_params \*p, const fb_cw2_params \*q, const double \*audio,", pub)
    assert re.search(r"int fb_debug_cw2_step\(fb_engine \*e, const fb_cw2_params \*q, int64_t N,", hooks)
    body = pub[pub.rindex("typedef struct {", 0, pub.index("} fb_cw2_params;")):pub.index("} fb_cw2_params;")]
    names = []
    for decl in body.replace("typedef struct {", "").split(";"):
        if decl.strip():
            typ, rest = decl.strip().split(None, 1)
            names += [(typ, n.strip()) for n in rest.split(",")]
    assert [n for _, n in names] == [f[0] for f in N.Cw2Params._fields_]
    for (typ, _n), (_f, ft) in zip(names, N.Cw2Params._fields_):
        assert {"double": "c_double", "int": "c_int"}[typ] == ft.__name__
    for word in ("tanh", "atanh(0.999999", "adver_loss < 0", "0.9999*prev", "ascending block order", "h = 128, 64, 32, 16, 8, 4, 2, 1",
                 "companions, an air channel, feature compression, dither > 0", "SpeakerGuard's CW2 reads a decision"):
        assert word in pub, word
    lib = C.CDLL(N.LIB_PATH)
    for name in ("fb_attack_cw2", "fb_debug_cw2_step"):
        assert name in N.EXPORTS
        getattr(lib, name)


def test_defaults_and_signatures():
    q = cw2_params()
    assert (q.initial_const, q.search_steps, q.lr, q.beta1, q.beta2, q.adam_eps, q.abort_every) == (1e-3, 9, 1e-2, 0.9, 0.999, 1e-8, 1000)
    assert list(inspect.signature(Engine.attack_cw2).parameters) == ["self", "params", "cw2", "audio"]
    sig = inspect.signature(CW2.__init__).parameters
    assert list(sig) == ["self", "task", "attack_type", "model", "confidence", "initial_const", "binary_search_steps", "max_iter", "lr",
                         "stop_early", "stop_early_iter", "bpda", "eot_size", "ivector", "seed", "verbose"]
    assert [sig[k].default for k in list(sig)[4:]] == [0., 1e-3, 9, 10000, 1e-2, True, 1000, False, 1, False, None, True]
    pa, ca = inspect.signature(PGD.attack).parameters, inspect.signature(CW2.attack).parameters
    assert list(pa) == list(ca) and all(pa[k].default == ca[k].default for k in pa)


class _Engine(object):
    kind = "gmm"

    def __init__(self, S):
        self.n_speakers, self.calls = S, []

    def attack_cw2(self, p, q, audio):
        self.calls.append((p.samples_per_draw, p.max_iter, p.threshold, p.target, p.adver_thresh, p.bits_per_sample, p.seed, p.stream,
                           q.initial_const, q.search_steps, q.lr, q.beta1, q.beta2, q.adam_eps, q.abort_every))
        S = max(self.n_speakers, 1)
        trace = np.arange(5 * (3 + S), dtype=np.float64).reshape(5, 3 + S)
        adv = R.cast_i16(audio, p.bits_per_sample)
        adv[:4] += 3
        return dict(adv=adv, success=1, adver_f64=audio.copy(), trace=trace, rows_per_step=np.array([3, 2], np.int32), best_l2=0.125,
                    const=5e-4)

    def attack_iter_seconds(self, n):
        return 0.25 * (1 + np.arange(n))

    def set_eot(self, r):
        self.calls.append(("eot", r))

    def set_wb_bpda(self, on):
        self.calls.append(("bpda", on))

    def set_wb_ivector(self, on):
        self.calls.append(("ivector", on))


class _Model(object):
    def __init__(self, task, S):
        self.task, self.engine = task, _Engine(S)


@pytest.mark.parametrize("task,S", [("OSI", 3), ("SV", 1)])
def test_cw2_marshals_and_writes_the_checkpoint(tmp_path, task, S):
    m = _Model(task, S)
    cw = CW2(task, "targeted", m, confidence=0.5, initial_const=0.25, binary_search_steps=2, max_iter=3, lr=0.125, stop_early_iter=7,
             seed=3, verbose=False)
    assert m.engine.calls == []                                 # no switch is touched without bpda / ivector
    audio = np.linspace(-0.5, 0.5, 40)
    cp = str(tmp_path / "a.cp")
    res = cw.attack(audio, cp, threshold=0.25, target=2 if task == "OSI" else None, bits_per_sample=16)
    adv, flag = res
    assert adv.dtype == np.int16 and adv.shape == (40, 1) and flag == 1
    assert m.engine.calls == [(0, 3, 0.25, 2 if task == "OSI" else 0, 0.5, 16, 0, 0, 0.25, 2, 0.125, 0.9, 0.999, 1e-8, 7)]
    assert res.best_l2 == 0.125 and res.const == 5e-4 and list(res.rows_per_step) == [3, 2]
    assert np.array_equal(res.perturbation_i16, [3] * 4 + [0] * 36)
    a0 = R.cast_i16(audio)
    assert res.snr_db == 10.0 * math.log10(float(np.sum(a0.astype(np.float64) ** 2)) / 36.0) == snr_db(a0, res.perturbation_i16)
    with open(cp, "rb") as r:
        rows = pickle.load(r)
    assert len(rows) == 5
    for k, row in enumerate(rows):                              # [l2, array([adver_loss]), score, used_time]
        assert len(row) == 4 and row[0] == k * (3 + S) and row[1].shape == (1,) and row[1][0] == k * (3 + S) + 1
        assert (np.ndim(row[2]) == 0 and row[2] == k * (3 + S) + 3) if task == "SV" else row[2].shape == (S,)
        assert row[3] == 0.25 * (k + 1)
    CW2(task, "targeted", m, stop_early=False, verbose=False).attack(audio, None)
    assert m.engine.calls[-1][-1] == 0 and m.engine.calls[-1][1] == 10000
    assert snr_db(a0, np.zeros(40)) == float("inf")


def test_cw2_switches_and_parameter_checks():
    m = _Model("OSI", 3)
    CW2("OSI", "targeted", m, bpda=True, eot_size=2, seed=5, verbose=False)
    assert m.engine.calls == [("eot", 2), ("bpda", True)]
    iv = _Model("OSI", 3)
    iv.engine.kind = "iv"
    with pytest.raises(ValueError, match="ivector=True"):
        CW2("OSI", "targeted", iv)
    CW2("OSI", "targeted", iv, ivector=True, verbose=False)
    assert iv.engine.calls == [("ivector", True)]
    with pytest.raises(ValueError, match="i-vector"):
        CW2("OSI", "targeted", iv, ivector=True, bpda=True, eot_size=2)
    with pytest.raises(ValueError):
        CW2("XYZ", "targeted", m)
    with pytest.raises(ValueError):
        CW2("SV", "targeted", m)
    with pytest.raises(TypeError):
        CW2("OSI", "targeted", object())
    for kw, word in ((dict(binary_search_steps=0), "binary_search_steps"), (dict(binary_search_steps=33), "binary_search_steps"),
                     (dict(initial_const=0.0), "initial_const"), (dict(initial_const=float("nan")), "initial_const"),
                     (dict(lr=-1.0), "lr"), (dict(lr=float("inf")), "lr"), (dict(max_iter=0), "max_iter"),
                     (dict(binary_search_steps=32, max_iter=2 ** 26), "2\\^30"), (dict(stop_early_iter=0), "stop_early_iter"),
                     (dict(eot_size=2), "bpda=True"), (dict(eot_size=33, bpda=True), "eot_size")):
        with pytest.raises(ValueError, match=word):
            CW2("OSI", "targeted", _Model("OSI", 3), **kw)
    check_cw2_params(1e-3, 9, 10000, 1e-2, 1000)
    assert "exactly as PGD.estimate_threshold does" in CW2.estimate_threshold.__doc__


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
    err = io.StringIO()
    with contextlib.redirect_stdout(io.StringIO()), contextlib.redirect_stderr(err):
        try:
            res = AM.main(argv, model_factory=model, bob_factory=bob)
        except SystemExit:
            raise SystemExit(err.getvalue())
    return res, seen


def test_attack_main_hands_cw2_its_options(site):
    (g, results, _thr), seen = _main(["--attack", "cw2", "-max_iter", "40", "-adver", "0.5", "--cw2-const", "0.01", "--cw2-steps", "3",
                                      "--cw2-lr", "0.002", "--cw2-abort-every", "10", "-epsilon", "0.004"])
    assert seen == [dict(confidence=0.5, initial_const=0.01, binary_search_steps=3, max_iter=40, lr=0.002, stop_early=True,
                         stop_early_iter=10)]
    assert g[1] == len(results) > 0
    _res, seen = _main(["--attack", "cw2", "--cw2-abort-every", "0", "--bpda", "--eot-size", "2", "--input-transform", "qt:512"])
    assert seen[0]["stop_early"] is False and seen[0]["bpda"] is True and seen[0]["eot_size"] == 2
    _res, seen = _main(["--attack", "cw2", "-archi", "iv", "--wb-ivector"])
    assert seen[0]["ivector"] is True and "bpda" not in seen[0]


@pytest.mark.parametrize("extra,word", [
    (["--companions", "1"], "companion"), (["--air-channel", "t60:200-600"], "--air-channel"), (["--feco", "0.5"], "--feco"),
    (["--dither", "1.0"], "--dither"), (["--bpda", "--air-channel", "t60:200-600"], "--air-channel"), (["--bpda", "--feco", "0.5"], "--feco"),
    (["--bpda", "--dither", "1.0"], "--dither"), (["--bpda", "--companions", "1"], "companion"), (["--input-transform", "ms:7"], "--bpda"),
    (["--codec", "ulaw"], "--bpda"), (["--eot-size", "2"], "--bpda"), (["-archi", "iv"], "--wb-ivector"),
    (["-archi", "iv", "--wb-ivector", "--bpda", "--eot-size", "2"], "--eot-size"), (["--wb-air"], "--wb-air"),
    (["--wb-frontend"], "--wb-frontend"), (["--wb-universal"], "--wb-universal"), (["--cw2-steps", "0"], "binary_search_steps"),
    (["--cw2-steps", "33"], "binary_search_steps"), (["--cw2-const", "0"], "initial_const"), (["--cw2-lr", "-1"], "lr"),
    (["--cw2-abort-every", "-1"], "--cw2-abort-every"), (["-max_iter", "0"], "max_iter")])
def test_attack_main_refuses_cw2_with_a_message_before_any_model_is_built(site, extra, word):
    built = []
    with pytest.raises(SystemExit) as ex:
        _main(["--attack", "cw2"] + extra, built)
    assert built == [] and word in str(ex.value), str(ex.value)
