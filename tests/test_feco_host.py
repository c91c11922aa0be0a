"""Feature compression without a GPU: the numpy restatement of the stage contract (tests/feco_ref.py) against scipy's k-means
and on the cases with a known answer, the spec parser, the system classes' keyword / FB_FECO, --feco reaching make_model, and
the library's new symbols."""
import inspect

import numpy as np
import pytest

from fakebob_amd import _native, systems
from tests.feco_ref import feco, feco_assign, feco_init, feco_k, feco_keys

D = 72


def _clusters(n_clusters, per, seed):
    """well-separated clusters: unit-variance points around centres at least 20 sigma apart in every pair"""
    rng = np.random.RandomState(seed)
    centres = np.zeros((n_clusters, D), np.float32)
    for c in range(n_clusters):
        centres[c, c % D] = 40.0 * (1 + c // D)      # distinct axes: pairwise distance >= 40 * sqrt(2)
    lab = np.repeat(np.arange(n_clusters), per)
    rng.shuffle(lab)
    X = (centres[lab] + rng.standard_normal((lab.size, D))).astype(np.float32)
    return X, lab


@pytest.mark.parametrize("iters", [1, 10])
def test_restatement_against_scipy_kmeans2(iters):
    vq = pytest.importorskip("scipy.cluster.vq")
    X, lab = _clusters(6, 25, 3)
    init = sorted(int(np.flatnonzero(lab == c)[0]) for c in range(6))        # one frame of every cluster
    C, labels = feco(X, None, 6.0 / X.shape[0], iters, init=init)
    want_c, want_l = vq.kmeans2(X.astype(np.float64), X[init].astype(np.float64), iter=iters, minit="matrix")
    assert np.array_equal(labels, want_l)
    assert np.abs(C.astype(np.float64) - want_c).max() <= 1e-5
    assert len(set(labels.tolist())) == 6


def test_k_is_one_product_and_one_floor():
    assert [feco_k(T, 0.5) for T in (0, 1, 2, 3, 300)] == [0, 1, 1, 1, 150]
    assert feco_k(300, 0.001) == 1 and feco_k(300, 1.0) == 300 and feco_k(257, 0.2) == 51
    assert feco_k(10, 0.3) == int(np.floor(np.float64(10) * np.float64(0.3)))


def test_keys_take_word_t_and_3_and_selection_is_by_key_then_frame(oracle):
    seed, stream, epoch, utt, rep = 0x1234567890ABCDEF, 7, 3, 2, 1
    keys = feco_keys(oracle.philox, seed, stream, epoch, utt, rep, 10)
    key = [(seed & 0xFFFFFFFF) ^ 0x4645434F, (seed >> 32) ^ stream]
    for t in (0, 3, 4, 9):
        assert int(keys[t]) == oracle.philox([t >> 2, 0x100 + rep, utt, epoch], key)[t & 3]
    assert not np.array_equal(keys, feco_keys(oracle.philox, seed, stream, epoch, utt, 0, 10))       # the replica counts
    assert feco_init(np.array([5, 1, 5, 0, 1], np.uint32), 3) == [1, 3, 4]                           # (0, 3) (1, 1) (1, 4)
    assert feco_init(np.array([5, 1, 5, 0, 1], np.uint32), 4) == [0, 1, 3, 4]                        # then (5, 0) before (5, 2)


def test_ratio_one_returns_the_input():
    rng = np.random.RandomState(5)
    X = rng.standard_normal((37, D)).astype(np.float32)
    X[20] = X[4]                                           # a repeated row: its second centre stays empty and keeps its value
    C, labels = feco(X, rng.randint(0, 2 ** 32, 37, dtype=np.uint64).astype(np.uint32), 1.0, 10)
    assert np.array_equal(C, X)
    assert labels[20] == 4 and 20 not in labels


def test_one_centre_is_the_float64_mean():
    rng = np.random.RandomState(6)
    X = (100.0 * rng.standard_normal((65, D))).astype(np.float32)
    C, labels = feco(X, np.arange(65, dtype=np.uint32), 0.001, 3)
    S = np.zeros(D, np.float64)
    for t in range(65):
        S = S + X[t].astype(np.float64)
    assert C.shape == (1, D) and np.array_equal(C[0], (S / 65.0).astype(np.float32))
    assert not labels.any()


def test_duplicated_rows_leave_an_empty_cluster_that_keeps_its_centre():
    rng = np.random.RandomState(7)
    X = rng.standard_normal((8, D)).astype(np.float32)
    X[1] = X[0]
    X[2:] += 50.0                                                   # (the other frames: far away, centre 2's)
    keys = np.array([0, 1, 2, 9, 9, 9, 9, 9], np.uint32)            # frames 0, 1, 2 start the three centres
    assert np.array_equal(feco_assign(X, X[[0, 1, 2]])[:3], [0, 0, 2])   # the tie goes to the lower centre
    C, labels = feco(X, keys, 3.0 / 8.0, 10)
    assert 1 not in labels
    assert np.array_equal(C[1], X[1])


def test_spec_parsing():
    assert systems.parse_feco("0.5") == (0.5, 10)
    assert systems.parse_feco("0.5:10") == (0.5, 10)
    assert systems.parse_feco(" 0.2:3 ") == (0.2, 3)
    assert systems.parse_feco(0.25) == (0.25, 10) and systems.parse_feco((1.0, 64)) == (1.0, 64)
    assert systems.parse_feco("none") is None and systems.parse_feco("off") is None
    for junk in ("", "abc", "0.5:", "0.5:x", "0.5:10:2", "0", "-0.1", "1.5", "nan", "0.5:0", "0.5:65", "0.5:1.5"):
        with pytest.raises(ValueError):
            systems.parse_feco(junk)


def test_system_classes_take_the_keyword_and_the_environment(monkeypatch):
    for cls in (systems.gmm_OSI, systems.gmm_CSI, systems.gmm_SV, systems.iv_OSI, systems.iv_CSI, systems.iv_SV):
        assert inspect.signature(cls.__init__).parameters["feature_compression"].default is None
    from fakebob_amd.dropin import gmm_ubm_OSI
    assert "feature_compression" in inspect.signature(gmm_ubm_OSI.gmm_OSI.__init__).parameters       # the drop-ins inherit it

    class Eng(object):
        got = "untouched"

        def set_feature_compression(self, ratio, iters=10):
            self.got = (ratio, iters) if ratio is not None else None
    monkeypatch.delenv("FB_FECO", raising=False)
    e = Eng()
    systems.apply_feature_compression(e, None)
    assert e.got == "untouched"                       # nothing asked for: the engine keeps its setting
    systems.apply_feature_compression(e, "0.5")
    assert e.got == (0.5, 10)
    monkeypatch.setenv("FB_FECO", "0.2:4")
    systems.apply_feature_compression(e, None)
    assert e.got == (0.2, 4)
    systems.apply_feature_compression(e, "none")      # the keyword wins over the environment
    assert e.got is None
    monkeypatch.setenv("FB_FECO", "junk")
    with pytest.raises(ValueError):
        systems.apply_feature_compression(e, None)


def test_feco_option_reaches_make_model(monkeypatch, tmp_path):
    from fakebob_amd import attack_main

    class Reached(Exception):
        pass
    seen = {}

    def fake_make_model(architecture, task, model_list, pre_model_dir, threshold, group_id, **kw):
        seen.update(kw)
        raise Reached()
    assert "feature_compression" in inspect.signature(attack_main.make_model).parameters
    monkeypatch.setattr(attack_main, "make_model", fake_make_model)
    monkeypatch.setattr(attack_main, "load_spk_models", lambda *a, **k: [])
    with pytest.raises(Reached):
        attack_main.main(["-spk_id", "a", "--feco", "0.5:10", "--out_dir", str(tmp_path)])
    assert seen == {"feature_compression": "0.5:10"}


def test_the_library_exports_the_new_symbols():
    names = ("fb_set_feature_compression", "fb_debug_feature_compress", "fb_debug_feco_keys")
    L = _native.lib()
    for name in names:
        assert name in _native.EXPORTS
        assert hasattr(L, name), name
    import ctypes as C
    assert L.fb_set_feature_compression(None, C.c_double(0.5), C.c_int(10)) == _native.FB_E_ARG      # (a null engine is refused, not followed)
