"""Input-transform chains without a GPU: the spec parser and the stage builders, the limits refused in Python before the
call, the ctypes struct against the header, and sanity checks of the numpy restatement (tests/input_transform_ref.py) the
GPU tests hold the kernel to."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from fakebob_amd import _native
from fakebob_amd import input_transform as T
from tests.input_transform_ref import DECIMATE, FIR, MEDIAN, QUANT, ref, ref_stage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _x(n, seed=0):
    rng = np.random.default_rng(seed)
    x = rng.integers(-32768, 32768, n).astype(np.int16)
    x[n // 3:n // 3 + 40] = 32767
    x[n // 2:n // 2 + 40] = -32768
    return x


# ---------------------------------------------------------------------------------------------------- parser, builders
def test_kind_codes_match_the_header_and_the_restatement():
    hdr = open(os.path.join(ROOT, "include", "fakebob_hip.h")).read()
    m = re.search(r"enum \{ FB_TF_QUANT = (\d), FB_TF_MEDIAN = (\d), FB_TF_FIR = (\d), FB_TF_DECIMATE = (\d) \};", hdr)
    want = tuple(int(v) for v in m.groups())
    assert want == (T.QUANT, T.MEDIAN, T.FIR, T.DECIMATE) == (QUANT, MEDIAN, FIR, DECIMATE)
    assert want == (_native.FB_TF_QUANT, _native.FB_TF_MEDIAN, _native.FB_TF_FIR, _native.FB_TF_DECIMATE)


def test_ctypes_stage_matches_the_header_field_order():
    hdr = open(os.path.join(ROOT, "include", "fakebob_hip.h")).read()
    m = re.search(r"typedef struct \{([^}]*)\} fb_tf_stage;", hdr)
    fields = [d.strip() for d in m.group(1).split(";") if d.strip()]
    assert fields == ["int kind", "int k", "const double *taps"]
    assert [f[0] for f in _native.TfStage._fields_] == ["kind", "k", "taps"]
    assert [f[1] for f in _native.TfStage._fields_] == [C.c_int, C.c_int, C.POINTER(C.c_double)]
    assert _native.TfStage.taps.offset == 8 and C.sizeof(_native.TfStage) == 16
    assert "fb_set_input_transform" in _native.EXPORTS and "fb_debug_input_transform" in _native.EXPORTS


def test_spec_parser():
    assert T.parse(None) == [] and T.parse("") == [] and T.parse("none") == []
    ch = T.parse("ms:7,qt:512")
    assert [(s.kind, s.k) for s in ch] == [(T.MEDIAN, 7), (T.QUANT, 512)] and all(s.taps is None for s in ch)
    ch = T.parse(" dec:3 , as:5 ")
    assert (ch[0].kind, ch[0].k) == (T.DECIMATE, 3)
    assert ch[1].kind == T.FIR and ch[1].k == 5 and np.array_equal(ch[1].taps, np.full(5, 1.0 / 5))
    ds = T.parse("ds:2")
    assert [(s.kind, s.k) for s in ds] == [(T.FIR, 101), (T.DECIMATE, 2), (T.FIR, 101)]
    assert abs(ds[0].taps.sum() - 1.0) < 1e-12 and abs(ds[2].taps.sum() - 2.0) < 1e-12   # the gain q sits in the second filter
    assert np.array_equal(ds[0].taps, ds[0].taps[::-1])                                 # linear phase
    assert [(s.kind, s.k) for s in T.parse("ds:4:31")] == [(T.FIR, 31), (T.DECIMATE, 4), (T.FIR, 31)]
    lp = T.parse("lpf:4000")
    assert len(lp) == 1 and lp[0].kind == T.FIR and lp[0].k == 101 and lp[0].taps.dtype == np.float64
    H = np.abs(np.fft.rfft(lp[0].taps, 1600))                                            # 10 Hz bins
    assert abs(H[0] - 1.0) < 1e-12 and H[:300].min() > 0.9 and H[520:].max() < 0.01
    assert T.parse("lpf:2000:51")[0].k == 51
    assert T.parse([T.median(3), [T.quant(2), T.decimate(2)]]) == [T.median(3), T.quant(2), T.decimate(2)]
    assert T.parse(T.quant(8)) == [T.quant(8)]
    for bad in ("ms", "ms:4", "xx:3", "qt:0", "qt:16385", "ms:33", "dec:1", "dec:65", "as:4", "lpf:9000", "ms:7;qt:2",
                "qt:1.5"):
        with pytest.raises(ValueError):
            T.parse(bad)


def test_limits_are_refused_before_the_call():
    with pytest.raises(ValueError):
        T.parse(",".join(["qt:2"] * 9))                                    # 9 stages
    assert len(T.parse(",".join(["qt:2"] * 8))) == 8
    t511 = np.zeros(511)
    t511[255] = 1.0
    assert sum(T.radius(s) for s in T.validate([T.fir(t511)] * 4 + [T.median(9)])) == 1024
    with pytest.raises(ValueError):
        T.validate([T.fir(t511)] * 4 + [T.median(11)])                     # radii sum to 1025
    for bad in (np.ones(513), np.ones(4), np.array([np.nan]), np.array([np.inf]), np.array([2.0 ** 20 + 1.0]), np.ones(0)):
        with pytest.raises(ValueError):
            T.fir(bad)
    assert T.fir([2.0 ** 20]).k == 1 and T.fir(np.ones(511)).k == 511
    for bad in (T.Stage(T.MEDIAN, 4, None), T.Stage(T.QUANT, 0, None), T.Stage(T.DECIMATE, 1, None), T.Stage(9, 3, None),
                T.Stage(T.FIR, 3, np.ones(5))):
        with pytest.raises(ValueError):
            T.validate([bad])
    with pytest.raises(TypeError):
        T.validate([(T.QUANT, 2, None)])


def test_engine_refuses_in_python_before_the_native_call():
    """Engine.set_input_transform validates first: the library is never reached with a chain outside the limits."""
    from fakebob_amd.engine import Engine

    class Lib(object):
        def fb_set_input_transform(self, *a):
            raise AssertionError("reached the library")
    e = Engine.__new__(Engine)
    e._L, e._h = Lib(), C.c_void_p()
    for bad in ("ms:4", ",".join(["qt:2"] * 9), [T.Stage(T.QUANT, 0, None)]):
        with pytest.raises(ValueError):
            e.set_input_transform(bad)


def test_c_stages_carries_the_taps_as_data():
    ch = T.parse("qt:4,as:3")
    arr, keep = T.c_stages(ch)
    assert (arr[0].kind, arr[0].k, bool(arr[0].taps)) == (T.QUANT, 4, False)
    assert (arr[1].kind, arr[1].k) == (T.FIR, 3) and [arr[1].taps[j] for j in range(3)] == [1.0 / 3] * 3
    assert len(keep) == 1


def test_system_classes_take_the_keyword_and_the_environment(monkeypatch):
    import inspect
    from fakebob_amd import systems
    for cls in (systems.gmm_OSI, systems.gmm_CSI, systems.gmm_SV, systems.iv_OSI, systems.iv_CSI, systems.iv_SV):
        assert inspect.signature(cls.__init__).parameters["input_transform"].default is None

    class Eng(object):
        got = "untouched"

        def set_input_transform(self, spec):
            self.got = spec
    monkeypatch.delenv("FB_INPUT_TRANSFORM", raising=False)
    e = Eng()
    systems._apply_input_transform(e, None)
    assert e.got == "untouched"                       # nothing asked for: the engine keeps its chain
    systems._apply_input_transform(e, "ms:7")
    assert e.got == "ms:7"
    monkeypatch.setenv("FB_INPUT_TRANSFORM", "qt:512")
    systems._apply_input_transform(e, None)
    assert e.got == "qt:512"
    systems._apply_input_transform(e, "none")         # the keyword wins over the environment
    assert e.got == "none"


# ------------------------------------------------------------------------------------- the restatement's own sanity
@pytest.mark.parametrize("k", [3, 7, 31])
def test_ref_median_is_scipy_medfilt(k):
    from scipy.signal import medfilt
    for n in (1, 2, k - 1, k, 1000):
        x = _x(max(n, 1), seed=k)[:n]
        assert np.array_equal(ref_stage(x, MEDIAN, k), medfilt(x.astype(np.float64), k).astype(np.int16))


def test_ref_fir_single_unit_tap_is_the_identity():
    x = _x(5000)
    assert np.array_equal(ref_stage(x, FIR, 1, [1.0]), x)
    d = np.zeros(5)
    d[2] = 1.0
    assert np.array_equal(ref_stage(x, FIR, 5, d), x)
    d = np.zeros(5)
    d[1] = 1.0                                          # tap j = c - 1 reads x[i + 1]: an advance by one sample
    assert np.array_equal(ref_stage(x, FIR, 5, d), np.concatenate([x[1:], [0]]).astype(np.int16))


def test_ref_fir_rounds_ties_to_even_and_clips():
    x = np.array([1, 3, 5, -1, -3, 32767, -32768], np.int16)
    assert list(ref_stage(x, FIR, 1, [0.5])) == [0, 2, 2, 0, -2, 16384, -16384]
    assert list(ref_stage(x, FIR, 1, [2.0])) == [2, 6, 10, -2, -6, 32767, -32768]
    assert list(ref_stage(x, FIR, 1, [-2.0])) == [-2, -6, -10, 2, 6, -32768, 32767]


def test_ref_quant():
    x = _x(4000)
    for q in (1, 2, 128, 1000, 1024, 16384):
        y = ref_stage(x, QUANT, q)
        assert np.array_equal(ref_stage(y, QUANT, q), y)                                # idempotent
        inside = np.abs(y.astype(np.int64)) < 32767 - q
        assert np.all(y[inside].astype(np.int64) % q == 0)
        assert np.abs(y.astype(np.int64) - x)[inside].max() <= q // 2 + (q % 2)
    assert np.array_equal(ref_stage(x, QUANT, 1), x)
    assert list(ref_stage(np.array([-3, -2, -1, 0, 1, 2, 3, 32767, -32768], np.int16), QUANT, 4)) == \
        [-4, 0, 0, 0, 0, 4, 4, 32767, -32768]           # floor division of x + 2; 32768 clips


def test_ref_decimate_after_fir_equals_a_direct_computation():
    x = _x(300, seed=5)
    h = np.array([0.25, 0.5, 0.25])
    got = ref(x, [(FIR, 3, h), (DECIMATE, 3, None)])
    want = np.zeros(300, np.int16)
    for i in range(0, 300, 3):
        acc = 0.0
        for j in range(3):
            m = i + 1 - j
            acc = acc + h[j] * (float(x[m]) if 0 <= m < 300 else 0.0)
        want[i] = int(min(max(np.rint(acc), -32768), 32767))
    assert np.array_equal(got, want)


def test_ref_reads_zero_outside_the_utterance_at_every_stage():
    """Two box filters in a row: the second one reads zeros, not the first one's tail, beyond the ends."""
    x = np.full(4, 300, np.int16)
    box = np.ones(3)
    assert list(ref(x, [(FIR, 3, box)])) == [600, 900, 900, 600]
    assert list(ref(x, [(FIR, 3, box), (FIR, 3, box)])) == [1500, 2400, 2400, 1500]   # (the untruncated tail would add 300)
