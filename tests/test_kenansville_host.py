"""The decision-only attack without a GPU: the vectorised host twin (fakebob_amd/kenansville.py) against the plain-integer
restatement (tests/kenansville_ref.py) bit for bit, the contract's own bounds at the worst inputs, its agreement with a
float64 numpy.fft pipeline, the search on scripted decisions, then Kenansville's argument checks and attack_main's new flags
with stub models as tests/test_driver_rules.py uses them."""
import contextlib
import io
import os
import pickle

import numpy as np
import pytest

from fakebob_amd import attack_main as AM
from fakebob_amd import kenansville as KV
from tests import kenansville_ref as R
from tests.golden import driver_site as DS

WINDOWS = [8, 9, 33, 100, 127, 128]
FACTORS = [0, 1, 64, 6554, 65535, 65536]


def lengths(W):
    return [1, W - 1, W, W + 1, 3 * W + 5, 4099]


# ------------------------------------------------------------------------------------------------ the twin, bit for bit
@pytest.mark.parametrize("W", WINDOWS)
def test_tables_are_the_contracts(W):
    t = KV.tables(W)
    assert t.dtype == np.int32 and t.shape == (4, W) and t.flags["C_CONTIGUOUS"]
    assert [list(map(int, row)) for row in t] == [list(row) for row in R.tables(W)]
    assert (t[0, 0], t[1, 0], t[2, 0], t[3, 0]) == (1 << 30, 0, 1 << 22, 0)


@pytest.mark.parametrize("W", WINDOWS)
def test_remove_is_the_restatement_bit_for_bit(W):
    tab = R.tables(W)
    for n in lengths(W):
        x = R.edge_audio(W, n)
        wins, ans = R.analyse(x, W, tab)
        _X, a, b, cum, E = KV.analyse(x, W)
        assert a.tolist() == [an["a"] for an in ans] and b.tolist() == [an["b"] for an in ans]
        assert cum.tolist() == [an["cum"] for an in ans] and E.tolist() == [an["E"] for an in ans]
        for q in FACTORS:
            want = R.candidate(n, W, wins, ans, q, tab)
            got = KV.remove(x, W, q)
            assert got.dtype == np.int16 and got.shape == (n,)
            assert np.array_equal(got, want), (W, n, q, int(np.flatnonzero(got != want)[0]))
            if q == 0:
                assert np.array_equal(got, x)                                  # the identity, bit for bit


def test_a_silent_window_stays_silent_and_the_tie_rule_is_by_bin():
    W = 33
    x = R.edge_audio(W, 7 * W)
    for q in (1, 6554, 65536):
        assert not KV.remove(x, W, q)[W:2 * W].any()
    _wins, ans = R.analyse(x, W)
    assert len(set(ans[5]["p"])) == 1 and ans[5]["order"] == list(range(W // 2 + 1))   # the impulse: all p equal, order by k
    # the impulse's bins go one by one, lowest bin first
    got = [len(R.removed_bins(ans[5], q)) for q in (0, 65536 // 33 + 1, 3 * 65536 // 33 + 1, 65536)]
    assert got == [0, 1, 2, W // 2 + 1]


# ------------------------------------------------------------------------------------------------ bounds
def test_intermediates_stay_below_2_53_at_the_worst_inputs():
    W = 128
    tab = R.tables(W)
    worst = [np.full(W, -32768, np.int16), np.where(np.arange(W) % 2 == 0, -32768, 32767).astype(np.int16),
             np.where(np.arange(W) % 2 == 0, 32767, -32768).astype(np.int16)]
    for x in worst:
        _wins, ans = R.analyse(x, W, tab)
        big = max(max(abs(v) for v in ans[0]["A"]), max(abs(v) for v in ans[0]["B"]))
        assert big <= 2 ** 52
        assert max(max(abs(v) for v in ans[0]["a"]), max(abs(v) for v in ans[0]["b"])) <= 2 ** 22
        assert ans[0]["E"] < 2 ** 53 and max(ans[0]["cum"]) == ans[0]["E"]
        stats = {}
        y = R.remove(x, W, 65536, tab, stats)
        print("W = 128: max |A|, |B| = 2^%.3f, sum |terms of R| = 2^%.3f" % (np.log2(big), np.log2(stats["R_mag"])))
        assert stats["R_mag"] < 2 ** 53
        assert np.array_equal(KV.remove(x, W, 65536), y)
    _wins, ans = R.analyse(worst[0], W, tab)
    assert abs(ans[0]["A"][0]) == 2 ** 52                                      # the bound is attained
    # every window size: sum of |terms of R| for full-scale inputs
    for W in (8, 9, 33, 100, 127):
        for x in (np.full(W, -32768, np.int16), np.where(np.arange(W) % 2 == 0, -32768, 32767).astype(np.int16)):
            stats = {}
            R.remove(x, W, 65536, None, stats)
            assert stats["R_mag"] < 2 ** 53


# ------------------------------------------------------------------------------------------------ a float64 pipeline
def _utterance(n=6000, seed=12):
    """a fixed synthetic utterance with silent and full-scale stretches"""
    rng = np.random.RandomState(seed)
    t = np.arange(n)
    env = 0.55 + 0.45 * np.sin(2 * np.pi * t / 1700.0)
    v = env * (5000.0 * np.sin(2 * np.pi * 0.013 * t) + 3000.0 * np.sin(2 * np.pi * 0.071 * t + 0.4)
               + 1500.0 * np.sin(2 * np.pi * 0.19 * t + 1.1)) + rng.normal(0, 200.0, n)
    v[1000:1400] = 0.0                                                          # silence
    v[3000:3500] = rng.uniform(-1, 1, 500) * 40000.0                            # full scale, clipped
    return np.clip(np.rint(v), -32768, 32767).astype(np.int16)


def _float_pipeline(x, W, q):
    """numpy.fft.rfft / irfft in float64 with the contract's bin weights, a stable sort, threshold E q / 65536 and the clip
    -> (y float64 (N,), masks (nw, K) bool, doubtful (nw,) bool: a threshold comparison within 1e-9 relative)"""
    n = x.size
    nw, K = -(-n // W), W // 2 + 1
    X = np.zeros(nw * W)
    X[:n] = x
    X = X.reshape(nw, W)
    F = np.fft.rfft(X, axis=1)
    p = F.real ** 2 + F.imag ** 2
    e = KV.bin_weights(W)[None, :] * p
    E = e.sum(axis=1)
    order = np.argsort(p, axis=1, kind="stable")
    cs = np.cumsum(np.take_along_axis(e, order, 1), axis=1)
    cum = np.empty_like(cs)
    np.put_along_axis(cum, order, cs, 1)
    thr = E * q / 65536.0
    mask = cum <= thr[:, None]
    # (a silent window has E = 0 exactly, in floats as in integers: 0 <= 0 is no doubtful comparison)
    doubtful = ((np.abs(cum - thr[:, None]) <= 1e-9 * thr[:, None]) & (thr[:, None] > 0)).any(axis=1)
    y = X - np.fft.irfft(F * mask, n=W, axis=1)
    return np.clip(y, -32768.0, 32767.0).reshape(-1)[:n], mask, doubtful


@pytest.mark.parametrize("W", [8, 33, 100, 127, 128])
def test_agreement_with_a_float64_fft_pipeline(W):
    x = _utterance()
    tab = R.tables(W)
    _wins, ans = R.analyse(x, W, tab)
    worst = 0.0
    for q in (6554, 32768):                                                     # a tenth and a half of every window's energy
        y = KV.remove(x, W, q).astype(np.float64)
        yf, mask, doubtful = _float_pipeline(x, W, q)
        mine = np.zeros_like(mask)
        for w, an in enumerate(ans):
            mine[w, R.removed_bins(an, q)] = True
        left_out = int(doubtful.sum())
        print("W = %d, q = %d: %d of %d windows left out of the mask comparison" % (W, q, left_out, mask.shape[0]))
        assert left_out <= 0.01 * mask.shape[0]
        assert np.array_equal(mine[~doubtful], mask[~doubtful])
        worst = max(worst, float(np.abs(y - yf).max()))
    print("W = %d: max |y - y_float| = %.4f LSB" % (W, worst))
    assert worst <= 1.0


# ------------------------------------------------------------------------------------------------ the search
def _check_rounds(res, G, q_max, max_rounds, truth):
    """the invariants of a finished search; truth(q) -> whether q succeeds"""
    lo, hi = 0, None
    assert 1 <= len(res["rounds"]) <= max_rounds
    assert res["n_queries"] == sum(r["rows"] for r in res["rounds"])
    for i, r in enumerate(res["rounds"]):
        assert r["qs"] == sorted(set(r["qs"])) and len(r["qs"]) <= G and r["rows"] == len(r["qs"])
        assert all(lo < q and (hi is None or q < hi) for q in r["qs"]) and all(1 <= q <= q_max for q in r["qs"])
        if i > 0:
            d = hi - lo
            assert r["last"] == (d - 1 <= G)
            if r["last"]:
                assert r["qs"] == list(range(lo + 1, hi)) and i == len(res["rounds"]) - 1
        lo, hi = r["lo"], r["hi"]
        if hi is not None:
            assert lo < hi and truth(hi) and (lo == 0 or not truth(lo))        # lo failed, hi succeeded
    last = res["rounds"][-1]
    if res["success"] == 1:
        assert res["factor"] == hi
        assert hi - lo == 1 or last["last"] or len(res["rounds"]) == max_rounds
    else:
        assert len(res["rounds"]) == 1 and res["factor"] == -1 and hi is None


@pytest.mark.parametrize("G", [1, 2, 15, 64])
def test_search_on_a_monotone_victim_finds_the_edge(G):
    for edge in (1, 2, 3, 777, 6554, 40000, 65535, 65536):
        truth = lambda q: q >= edge                                             # noqa: E731
        res = R.search(lambda r, qs: [truth(q) for q in qs], G, 65536, 32)
        _check_rounds(res, G, 65536, 32, truth)
        assert (res["success"], res["factor"]) == (1, edge)                     # the smallest factor that succeeds
        if G == 1:
            assert len(res["rounds"]) <= 17 and all(r["rows"] <= 1 for r in res["rounds"])   # plain bisection


def test_search_with_g_1_is_bisection():
    seen = []
    R.search(lambda r, qs: seen.append(qs[0]) or [qs[0] >= 40000], 1, 65536, 32)
    assert seen[:4] == [65536, 32768, 49152, 40960]


def test_search_on_a_non_monotone_victim_keeps_its_invariant():
    rng = np.random.RandomState(5)
    good = set(int(v) for v in rng.randint(1, 65537, 3000)) | set(range(50000, 65537))
    truth = lambda q: q in good                                                 # noqa: E731
    for G in (1, 2, 15, 64):
        res = R.search(lambda r, qs: [truth(q) for q in qs], G, 65536, 32)
        _check_rounds(res, G, 65536, 32, truth)
        assert res["success"] == 1 and truth(res["factor"])


def test_search_that_never_succeeds_and_one_that_succeeds_at_once():
    for G in (1, 2, 15, 64):
        res = R.search(lambda r, qs: [False] * len(qs), G, 65536, 32)
        _check_rounds(res, G, 65536, 32, lambda q: False)
        assert (res["success"], res["factor"], res["n_queries"]) == (-1, -1, G)
        res = R.search(lambda r, qs: [True] * len(qs), G, 65536, 32)
        _check_rounds(res, G, 65536, 32, lambda q: True)
        assert (res["success"], res["factor"]) == (1, 1)
    # q_max below G: duplicates and zeros are dropped
    res = R.search(lambda r, qs: [False] * len(qs), 15, 4, 32)
    assert res["rounds"][0]["qs"] == [1, 2, 3, 4] and res["n_queries"] == 4
    res = R.search(lambda r, qs: [q >= 1 for q in qs], 64, 1, 32)
    assert res["rounds"][0]["qs"] == [1] and (res["factor"], len(res["rounds"])) == (1, 1)


def test_search_stops_at_max_rounds():
    truth = lambda q: q >= 12345                                                # noqa: E731
    res = R.search(lambda r, qs: [truth(q) for q in qs], 1, 65536, 5)
    _check_rounds(res, 1, 65536, 5, truth)
    assert len(res["rounds"]) == 5 and res["success"] == 1 and res["factor"] >= 12345


def test_no_decision_rows_never_succeed():
    # high factors approach silence: rows without voiced frames are decision -2, for targeted and untargeted goals alike
    assert R.decide("CSI", [0.1, 0.7, 0.7], 0.0) == 1 and R.decide("CSI", [0.1, 0.7], 0.0, tv=0) == -2
    assert R.decide("OSI", [0.1, 0.7, 0.7], 0.7) == 1 and R.decide("OSI", [0.1, 0.7, 0.7], 0.7000001) == -1
    assert R.decide("SV", [0.5], 0.5) == 1 and R.decide("SV", [0.4999], 0.5) == -1
    assert not R.succeeds(-2, "untargeted", 1) and not R.succeeds(-2, "targeted", -2)
    assert R.succeeds(-1, "untargeted", 1) and not R.succeeds(1, "untargeted", 1) and R.succeeds(2, "targeted", 2)
    # evasion at 20000, silence from 45000 on
    dec = lambda q: -2 if q >= 45000 else (0 if q >= 20000 else 1)              # noqa: E731
    truth = lambda q: R.succeeds(dec(q), "untargeted", 1)                       # noqa: E731
    res = R.search(lambda r, qs: [truth(q) for q in qs], 4, 65536, 32)
    _check_rounds(res, 4, 65536, 32, truth)
    assert res["rounds"][0]["flags"] == [False, True, False, False] and (res["success"], res["factor"]) == (1, 20000)


# ------------------------------------------------------------------------------------------------ Kenansville
class _Engine(object):
    """what Kenansville asks of an engine, with canned answers"""

    def __init__(self, S):
        self.S, self.calls = S, []

    def attack_kenansville(self, p, k, audio):
        self.calls.append(("kv", p.stream, p.seed, p.task, p.attack_type, p.threshold, p.target, p.true_label, p.bits_per_sample,
                           k.window, k.grid, k.q_max, k.max_rounds))
        G = k.grid
        qs = np.full((2, G), -1, np.int32)
        qs[0, :2], qs[1, :1] = [100, 200], [150]
        dec = np.zeros((2, G), np.int32)
        sc = np.arange(2 * G * self.S, dtype=np.float64).reshape(2, G, self.S)
        return dict(adv=np.arange(audio.size).astype(np.int16), success=1, factor=150, n_queries=3, qs=qs, decisions=dec,
                    scores=sc, trace=np.array([[100, 200, 2], [100, 150, 1]], np.int32))

    def attack_iter_seconds(self, n):
        return 0.25 * np.arange(1, n + 1)

    def estimate_threshold(self, p, model_threshold, audio, noise_all=None, max_total_iters=0):
        self.calls.append(("estimate", p.stream, p.seed, p.attack_type))
        return 1.5, 7, 2, 1.75, audio


class _Model(object):
    def __init__(self, task, S):
        self.task, self.threshold, self.engine = task, 0.5, _Engine(S)


def test_kenansville_checks_its_arguments():
    m = _Model("OSI", 3)
    kv = KV.Kenansville("OSI", "untargeted", m, seed=3, verbose=False)
    assert (kv.window, kv.grid, kv.q_max, kv.max_rounds) == (100, 15, 65536, 32) and kv.factor is None and kv.n_queries == 0
    assert KV.Kenansville("OSI", "untargeted", m, max_factor=0.5, verbose=False).q_max == 32768
    assert KV.Kenansville("OSI", "untargeted", m, max_factor=1e-9, verbose=False).q_max == 1
    with pytest.raises(ValueError, match="foreign"):
        KV.Kenansville("OSI", "untargeted", DS.StubModel("OSI"))                # score / make_decisions, no engine
    with pytest.raises(ValueError):
        KV.Kenansville("SV", "untargeted", m)                                   # the model's task is OSI
    bad = [dict(window=7), dict(window=129), dict(grid=0), dict(grid=65), dict(max_factor=0.0), dict(max_factor=1.0001),
           dict(max_factor=float("nan")), dict(max_factor=-0.5), dict(max_rounds=0), dict(max_rounds=33)]
    for kw in bad:
        with pytest.raises(ValueError):
            KV.Kenansville("OSI", "untargeted", m, **kw)
    with pytest.raises(ValueError):
        KV.Kenansville("XYZ", "untargeted", m)
    with pytest.raises(ValueError):
        KV.Kenansville("OSI", "sideways", m)
    for ok in (dict(window=8), dict(window=128), dict(grid=1), dict(grid=64), dict(max_rounds=1), dict(max_rounds=32)):
        KV.Kenansville("OSI", "untargeted", m, verbose=False, **ok)
    for fn in (lambda: KV.tables(7), lambda: KV.tables(129), lambda: KV.remove(np.zeros(8, np.int16), 8, -1),
               lambda: KV.remove(np.zeros(8, np.int16), 8, 65537), lambda: KV.remove(np.zeros(8, np.int16), 200, 1)):
        with pytest.raises(ValueError):
            fn()


@pytest.mark.parametrize("task,S", [("OSI", 3), ("SV", 1), ("CSI", 3)])
def test_kenansville_attack_marshals_and_writes_its_checkpoint(tmp_path, task, S):
    m = _Model(task, S)
    kv = KV.Kenansville(task, "untargeted", m, window=64, grid=4, max_factor=0.25, max_rounds=9, seed=11, verbose=False)
    audio = np.linspace(-0.5, 0.5, 40)
    cp = str(tmp_path / "a.cp")
    true = {"OSI": 2, "SV": None, "CSI": 1}[task]
    adv, flag = kv.attack(audio, cp, threshold=0.25, true=true, bits_per_sample=12)
    assert adv.dtype == np.int16 and adv.shape == (40, 1) and flag == 1 and kv.factor == 150 and kv.n_queries == 3
    want_true = 1 if task == "SV" else true                                     # for SV true=None means 1
    assert m.engine.calls == [("kv", 0, 11, {"OSI": 0, "CSI": 1, "SV": 2}[task], 0, 0.25, 0, want_true, 12, 64, 4, 16384, 9)]
    adv2, _ = kv.attack(audio[:, None], None, true=true)                        # a column, no checkpoint
    assert adv2.shape == (40, 1) and m.engine.calls[-1][1] == 1                 # the next stream, as FakeBob counts
    with open(cp, "rb") as r:
        rows = pickle.load(r)
    assert len(rows) == 2                                                       # one row per round
    assert rows[0][0].tolist() == [100, 200] and rows[1][0].tolist() == [150]
    assert rows[0][1].shape == (2,) and rows[0][2].shape == (2, S) and rows[1][2].shape == (1, S)
    assert rows[0][3:] == [100, 200, 0.25] and rows[1][3:] == [100, 150, 0.5]
    with pytest.raises(ValueError):
        kv.attack(audio, None, true=true, bits_per_sample=17)
    if task == "CSI":
        with pytest.raises(ValueError):
            kv.attack(audio, None)                                              # untargeted CSI needs the true speaker
        with pytest.raises(ValueError):
            KV.Kenansville(task, "targeted", m, verbose=False).attack(audio, None)


def test_kenansville_borrows_fakebobs_threshold_sweep(monkeypatch):
    monkeypatch.delenv("FB_EOT_SIZE", raising=False)
    m = _Model("OSI", 3)
    kv = KV.Kenansville("OSI", "untargeted", m, seed=11, verbose=False)
    kv._stream = 4
    assert kv.estimate_threshold(np.zeros(40))[:2] == (1.5, 7)
    assert m.engine.calls == [("estimate", 4, 11, 0)]
    assert kv.threshold == 1.75 and kv._stream == 5


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
    argv = ["-spk_id"] + DS.SPK_IDS + ["-task", "OSI", "-type", "untargeted", "--streams", "1", "--seed", "5"] + extra
    with contextlib.redirect_stdout(io.StringIO()), contextlib.redirect_stderr(io.StringIO()):
        res = AM.main(argv, model_factory=model, bob_factory=bob)
    return res, seen


def test_attack_main_hands_kenansville_its_options(site):
    (g, results, _thr), seen = _main(["--attack", "kenansville", "--kv-window", "64", "--kv-grid", "7", "--kv-max-factor", "0.5",
                                      "--eot-size", "1"])
    assert seen == [dict(window=64, grid=7, max_factor=0.5)]
    assert g[1] == len(results) > 0
    _res, seen = _main(["--attack", "kenansville"])
    assert seen == [dict(window=100, grid=15, max_factor=1.0)]
    for extra in ([], ["--attack", "nes"]):                                     # the default: nothing changes
        _res, seen = _main(extra)
        assert "window" not in seen[0] and "samples_per_draw" in seen[0]


@pytest.mark.parametrize("extra", [["--eot-size", "2"], ["--companions", "1"], ["--kv-window", "x"], ["--kv-grid", "1.5"],
                                   ["--kv-max-factor", "half"]])
def test_attack_main_refuses_before_any_model_is_built(site, extra):
    built = []
    with pytest.raises(SystemExit):
        _main(["--attack", "kenansville"] + extra, built)
    assert built == []
