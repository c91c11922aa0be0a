"""The telephone-line codecs without a GPU: the numpy restatement of the stage contract (tests/codec_ref.py) against code this
project did not write -- Python's audioop, through the golden file and directly where the interpreter still ships it --,
fakebob_amd.codec against the restatement, the lengths, the clamp row's coverage of the ADPCM state's four limits, and the
surface: names, the system classes' keyword / FB_CODEC, --codec reaching make_model.  Every comparison is np.array_equal."""
import contextlib
import inspect
import io
import os

import numpy as np
import pytest

from fakebob_amd import _native, attack_main as AM, codec as K, systems
from tests import codec_ref as R
from tests.golden import driver_site as DS

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "codec_audioop.npz")
ROWS = ("speech", "noise", "clamp")


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def _rand(n, seed, amp=32767):
    return np.random.default_rng(seed).integers(-amp - 1, amp + 1, n).astype(np.int16)


# ------------------------------------------------------------------------------------------- against audioop
def test_the_restatement_equals_the_golden_file(golden):
    allv = golden["all_values"]
    assert allv.dtype == np.int16 and np.array_equal(allv.astype(np.int32), np.arange(-32768, 32768))
    assert np.array_equal(R.ulaw(allv), golden["ulaw"])
    assert np.array_equal(R.alaw(allv), golden["alaw"])
    for name in ROWS:
        x = golden["adpcm_in_" + name]
        assert x.dtype == np.int16 and x.size % 2 == 0
        assert np.array_equal(R.adpcm(x), golden["adpcm_out_" + name]), name
    assert golden["adpcm_in_speech"].size == golden["adpcm_in_noise"].size == 4000
    assert np.array_equal(golden["adpcm_in_clamp"], R.clamp_row()) and R.clamp_row().size == 392


def test_the_restatement_equals_audioop(golden):
    audioop = pytest.importorskip("audioop")
    allv = golden["all_values"]
    raw = allv.tobytes()
    assert np.array_equal(R.ulaw(allv), np.frombuffer(audioop.ulaw2lin(audioop.lin2ulaw(raw, 2), 2), np.int16))
    assert np.array_equal(R.alaw(allv), np.frombuffer(audioop.alaw2lin(audioop.lin2alaw(raw, 2), 2), np.int16))
    rows = [golden["adpcm_in_" + name] for name in ROWS] + [_rand(1000, 1), _rand(1000, 2, amp=300), np.zeros(64, np.int16)]
    for i, x in enumerate(rows):
        code, _ = audioop.lin2adpcm(x.tobytes(), 2, None)
        y, _ = audioop.adpcm2lin(code, 2, None)
        assert np.array_equal(R.adpcm(x), np.frombuffer(y, np.int16)), i


def test_the_distortion_is_a_line_codecs(golden):
    """33 dB on the speech-like row, 16 dB on full-range noise through ADPCM, 37 dB through mu-law: the figures the codecs are
    known by, within a dB or two (the rows are this file's own, so the bounds are wide)"""
    def snr(x, y):
        x, y = x.astype(np.float64), y.astype(np.float64)
        return 10.0 * np.log10((x ** 2).sum() / ((x - y) ** 2).sum())
    sp, no = golden["adpcm_in_speech"], golden["adpcm_in_noise"]
    assert 28.0 < snr(sp, golden["adpcm_out_speech"]) < 38.0
    assert 12.0 < snr(no, golden["adpcm_out_noise"]) < 20.0
    assert 33.0 < snr(sp, R.ulaw(sp)) < 41.0 and 33.0 < snr(sp, R.alaw(sp)) < 41.0


# ------------------------------------------------------------------------------------------- the host module
def test_the_host_module_equals_the_restatement(golden):
    allv = golden["all_values"]
    assert np.array_equal(K.ulaw(allv), R.ulaw(allv)) and np.array_equal(K.alaw(allv), R.alaw(allv))
    rows = [golden["adpcm_in_" + name] for name in ROWS] + [_rand(777, 3), _rand(1, 4), np.zeros(33, np.int16)]
    for i, x in enumerate(rows):
        assert np.array_equal(K.adpcm(x), R.adpcm(x)), i
        for kind in R.KINDS:
            got = K.roundtrip(kind, x)
            assert got.dtype == np.int16 and np.array_equal(got, R.codec(kind, x)), (kind, i)
        assert np.array_equal(K.roundtrip(None, x), x) and np.array_equal(K.roundtrip("none", x), x)
    batch = np.stack([_rand(100, 5), _rand(100, 6)])
    assert np.array_equal(K.roundtrip("adpcm", batch), np.stack([R.adpcm(r) for r in batch]))   # every row on its own
    assert np.array_equal(K.roundtrip("ulaw", batch), R.ulaw(batch))
    assert K.STEP == R.STEP and K.IDX == R.IDX


@pytest.mark.parametrize("n", [1, 2, 3, 63, 64, 65, 511, 513])
def test_the_output_has_the_inputs_length(n):
    x = _rand(n, 10 + n)
    for kind in R.KINDS:
        for y in (R.codec(kind, x), K.roundtrip(kind, x)):
            assert y.shape == (n,) and y.dtype == np.int16, (kind, n)
    assert R.adpcm(x)[0] == R.adpcm(x[:1])[0]                                # causal: a prefix codes to the prefix
    assert np.array_equal(R.adpcm(x)[:n // 2], R.adpcm(x[:n // 2]))


def test_the_clamp_row_reaches_every_limit_of_the_state():
    """asserted on the restatement, so that a later change of the row cannot silently lose the coverage"""
    y, ix, raw = R.adpcm_trace(R.clamp_row())
    assert ix.min() == 0 and ix.max() == 88
    assert raw.max() > 32767 and raw.min() < -32768                         # the predictor runs into both clips ...
    assert y.max() == 32767 and y.min() == -32768                           # ... and is held there
    assert np.count_nonzero(ix[1:] == 0) > 1 and np.count_nonzero(ix == 88) > 1   # and the index is held at either end


def test_g711_properties():
    allv = np.arange(-32768, 32768, dtype=np.int32).astype(np.int16)
    for f, levels in ((R.ulaw, 255), (R.alaw, 256)):                        # mu-law's two zeros decode to one value
        y = f(allv)
        assert np.unique(y).size == levels
        assert np.all(np.diff(y.astype(np.int32)) >= 0)                     # monotone
        assert np.array_equal(f(y), y)                                      # a decoded value codes to itself
    assert R.ulaw(np.array([32767], np.int16))[0] == 32124 and R.ulaw(np.array([-32768], np.int16))[0] == -32124
    assert R.alaw(np.array([32767], np.int16))[0] == 32256 and R.alaw(np.array([-32768], np.int16))[0] == -32256
    assert R.alaw(np.array([0], np.int16))[0] == 8 and R.alaw(np.array([-1], np.int16))[0] == -8


# ------------------------------------------------------------------------------------------------ the surface
def test_names_and_kinds():
    assert (K.FB_CODEC_NONE, K.FB_CODEC_ULAW, K.FB_CODEC_ALAW, K.FB_CODEC_ADPCM) == (0, 1, 2, 3)
    assert [K.kind_of(n) for n in (None, "none", "", "ulaw", "ALAW", " adpcm ", 2)] == [0, 0, 0, 1, 2, 3, 2]
    assert [K.name_of(k) for k in (0, 1, 2, 3)] == [None, "ulaw", "alaw", "adpcm"]
    for bad in ("gsm", "mp3", 4, -1, 1.0, True):
        with pytest.raises(ValueError):
            K.kind_of(bad)
    for name in ("fb_set_codec", "fb_debug_codec"):
        assert name in _native.EXPORTS


def test_system_keyword_and_environment(monkeypatch):
    class FakeEngine(object):
        got = "untouched"

        def set_codec(self, codec):
            self.got = K.name_of(K.kind_of(codec))
    monkeypatch.delenv("FB_CODEC", raising=False)
    e = FakeEngine()
    systems._apply_codec(e, None)
    assert e.got == "untouched"                                             # nobody asked: the engine keeps its setting
    systems._apply_codec(e, "adpcm")
    assert e.got == "adpcm"
    monkeypatch.setenv("FB_CODEC", "ulaw")
    systems._apply_codec(e, None)
    assert e.got == "ulaw"
    systems._apply_codec(e, "none")                                         # the keyword wins over the environment
    assert e.got is None
    monkeypatch.setenv("FB_CODEC", "junk")
    with pytest.raises(ValueError):
        systems._apply_codec(e, None)
    for cls in (systems.gmm_OSI, systems.gmm_CSI, systems.gmm_SV, systems.iv_OSI, systems.iv_CSI, systems.iv_SV):
        assert "codec" in inspect.signature(cls.__init__).parameters, cls.__name__
    from fakebob_amd.dropin import gmm_ubm_OSI, ivector_PLDA_SV
    assert "codec" in inspect.signature(gmm_ubm_OSI.gmm_OSI.__init__).parameters
    assert "codec" in inspect.signature(ivector_PLDA_SV.iv_SV.__init__).parameters


def test_codec_option_reaches_make_model(monkeypatch, tmp_path):
    class Reached(Exception):
        pass
    seen = {}

    def fake_make_model(architecture, task, model_list, pre_model_dir, threshold, group_id, **kw):
        seen.update(kw)
        raise Reached()
    assert "codec" in inspect.signature(AM.make_model).parameters
    monkeypatch.setattr(AM, "make_model", fake_make_model)
    monkeypatch.setattr(AM, "load_spk_models", lambda *a, **k: [])
    for name in ("ulaw", "alaw", "adpcm", "none"):
        seen.clear()
        with pytest.raises(Reached):
            AM.main(["-spk_id", "a", "--codec", name, "--out_dir", str(tmp_path)])
        assert seen == {"codec": name}
    seen.clear()
    with pytest.raises(Reached):
        AM.main(["-spk_id", "a", "--out_dir", str(tmp_path)])
    assert "codec" not in seen                                              # not named: make_model's own default


@pytest.fixture()
def site(tmp_path):
    DS.make_site(str(tmp_path))
    old = os.getcwd()
    os.chdir(str(tmp_path))
    yield str(tmp_path)
    os.chdir(old)


def _main(extra, built):
    def bob(task, at, model, **hp):
        return DS.StubBob(task, at, model, **hp)

    def model(archi, t, ml, pre, th, gid):
        built.append(gid)
        return DS.StubModel(t, th)
    DS.StubBob.log = []
    argv = ["-spk_id"] + DS.SPK_IDS + ["-task", "OSI", "-type", "targeted", "--streams", "1", "--seed", "5"] + extra
    with contextlib.redirect_stdout(io.StringIO()), contextlib.redirect_stderr(io.StringIO()):
        return AM.main(argv, model_factory=model, bob_factory=bob)


@pytest.mark.parametrize("name", ["gsm", "opus", "ADPCM", ""])
def test_attack_main_refuses_an_unknown_codec_before_any_model_is_built(site, name):
    built = []
    with pytest.raises(SystemExit):
        _main(["--codec", name], built)
    assert built == []
    _main(["--codec", "adpcm"], built)                                      # a known name goes on to build the models
    assert built != []
