"""ParticleSwarm, Kenansville and HopSkipJump in front of a foreign model, without a GPU: the options they refuse by name, the
mode they pick for a model, and the numpy restatement of the decision rule (tests/foreign_attack_ref.decide_rows) against the
rule the native attacks are pinned to (tests/kenansville_ref.decide).  No engine is created."""
import numpy as np
import pytest

from fakebob_amd import foreign as FG
from fakebob_amd.hsj import HopSkipJump
from fakebob_amd.kenansville import Kenansville
from fakebob_amd.pso import ParticleSwarm
from tests import foreign_attack_ref as FR
from tests.golden.synth_model import SynthModel
from tests.kenansville_ref import decide

CLASSES = [ParticleSwarm, Kenansville, HopSkipJump]


@pytest.mark.parametrize("cls", CLASSES)
def test_a_foreign_model_refuses_the_engines_options_by_name(cls):
    m = SynthModel("SV", 1, 64)
    for kw, name in ((dict(eot_size=2), "eot_size"), (dict(eot_size=2, quorum="majority"), "eot_size"), (dict(quorum=1), "quorum"),
                     (dict(quorum="majority"), "quorum"), (dict(play_offset=3), "play_offset")):
        with pytest.raises(ValueError, match=name):
            cls("SV", "untargeted", m, verbose=False, foreign=True, **kw)
    with pytest.raises(ValueError, match="foreign=True"):                        # unasked, a model without an engine is refused as before
        cls("SV", "untargeted", m, verbose=False)
    a = cls("SV", "untargeted", m, verbose=False, eot_size=1, foreign=True)                    # (one draw is no option)
    assert a._victim is not None and a._victim._engine is None
    with pytest.raises(ValueError, match="companions"):
        a.attack(np.zeros(64), None, true=1, companions=[np.zeros(64)], init=np.zeros(64)) if cls is HopSkipJump else \
            a.attack(np.zeros(64), None, true=1, companions=[np.zeros(64)])
    assert a._victim._engine is None                                             # refused before any engine exists


class _Score(object):
    task, spk_ids = "CSI", ["a", "b"]

    def score(self, audios, **kw):
        raise AssertionError("not called")


class _Decide(object):
    task, spk_ids = "CSI", ["a", "b"]

    def make_decisions(self, audios, **kw):
        raise AssertionError("not called")


class _Both(_Score, _Decide):
    pass


class _Device(_Both):
    def score_device(self, x):
        raise AssertionError("not called")


@pytest.mark.parametrize("cls", CLASSES)
def test_the_mode_follows_the_model(cls):
    reads_decisions = cls is not ParticleSwarm
    want = {_Score: FG.HOST_SCORES, _Decide: FG.HOST_DECISIONS if reads_decisions else None,
            _Both: FG.HOST_DECISIONS if reads_decisions else FG.HOST_SCORES, _Device: FG.DEVICE_SCORES}
    for kind, mode in want.items():
        if mode is None:                                                         # PSO reads scores: make_decisions alone is no model
            with pytest.raises(TypeError):
                cls("CSI", "untargeted", kind(), verbose=False, foreign=True)
            continue
        a = cls("CSI", "untargeted", kind(), verbose=False, foreign=True)
        assert a._victim.mode == mode and a._victim.device == (kind is _Device)
        assert a._victim.speakers(None) == 2 and a._victim._engine is None       # spk_ids: FakeBob._speakers' rule
    with pytest.raises(TypeError):
        cls("CSI", "untargeted", object(), verbose=False, foreign=True)


def test_speakers_follow_fakebobs_rule():
    from fakebob_amd.attack import FakeBob, model_speakers
    assert model_speakers(object(), "SV") == 1
    assert model_speakers(_Score(), "OSI") == 2
    with pytest.raises(ValueError, match="spk_ids"):
        model_speakers(object(), "OSI")
    assert model_speakers(object(), "OSI", np.zeros((4, 1)), lambda a: 5) == 5
    m = SynthModel("CSI", 3, 16)
    del m.spk_ids
    fb = FakeBob("CSI", "untargeted", m, verbose=False)
    assert fb._speakers(np.zeros((16, 1))) == 3 and m.n_calls == 1               # the width of ONE extra score call


def _edge_rows(S, dtype):
    """all scores equal; a maximum exactly at the threshold (0.5); a NaN in column 0; a NaN elsewhere; ties; random rows"""
    rs = np.random.RandomState(S)
    rows = [np.full(S, 0.25), np.full(S, 0.5), np.full(S, -0.0)]
    r = rs.uniform(-1.0, 0.4, S); r[S // 2] = 0.5; rows.append(r)                # the maximum exactly at the threshold
    r = rs.uniform(-1.0, 1.0, S); r[0] = np.nan; rows.append(r)                  # a NaN in column 0 stays the running maximum
    r = rs.uniform(-1.0, 1.0, S); r[S - 1] = np.nan; rows.append(r)              # a NaN elsewhere never displaces it
    r = rs.uniform(-1.0, 0.0, S); r[S - 1] = r[S // 3] = 0.75; rows.append(r)    # a tie: the first maximum
    rows.append(np.full(S, np.nan))
    rows.append(np.full(S, np.float32(0.5) - np.float32(2.0 ** -25)))            # below the threshold in float64, not in float32
    rows += [rs.normal(0.5, 0.3, S) for _ in range(8)]
    return np.array(rows).astype(dtype)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_the_decision_rule_is_the_native_one(dtype):
    for task, sizes in (("SV", [1]), ("OSI", [1, 2, 3, 61]), ("CSI", [1, 2, 3, 61])):
        for S in sizes:
            sc = _edge_rows(S, dtype)
            dec, wide = FR.decide_rows(task, sc, 0.5)
            assert wide.dtype == np.float64 and np.array_equal(wide, sc.astype(np.float64), equal_nan=True)
            assert dec.dtype == np.int32 and dec.tolist() == [decide(task, row, 0.5) for row in wide]
            assert dec.tolist() == FG.decide_scores(task, wide, 0.5)             # the product's host twin (noise starts)
    # the cases by hand
    assert FR.decide_rows("SV", [[0.5], [np.nextafter(0.5, 0.0)], [np.nan]], 0.5)[0].tolist() == [1, -1, -1]
    assert FR.decide_rows("CSI", [[1.0, 1.0, 1.0], [0.0, 2.0, 2.0], [np.nan, 9.0, 9.5], [1.0, np.nan, 0.5]], 0.5)[0].tolist() == [0, 1, 0, 0]
    assert FR.decide_rows("OSI", [[0.5, 0.1], [0.4, 0.1], [np.nan, 0.9], [0.1, np.nan]], 0.5)[0].tolist() == [0, -1, 0, -1]
    # float32 widening: the float32 nearest to 0.5 - 2^-26 IS 0.5, so it passes a float64 threshold of 0.5
    assert FR.decide_rows("SV", np.array([[0.5 - 2.0 ** -26]], np.float32), 0.5)[0].tolist() == [1]
    assert FR.decide_rows("SV", np.array([[0.5 - 2.0 ** -26]], np.float64), 0.5)[0].tolist() == [-1]


def test_what_the_victim_sees_is_exact():
    q = np.array([[-32768, -1, 0, 1, 32767]], np.int16)
    for bits in (16, 8):
        x64, x32 = FR.rows_to_model(q, bits), FR.rows_to_model(q, bits, np.float32)
        assert np.array_equal(x32.astype(np.float64), x64)
        assert np.array_equal((x64 * 2.0 ** (bits - 1)).astype(np.int64), q.astype(np.int64))
