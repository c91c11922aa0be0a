"""The voted decision on the host: the numpy restatement (tests/vote_ref.py) on hand-made cases, the quorum rules of
fakebob_amd.query_eot, and the Python attack classes' refusal of eot_size > 1 without a quorum -- before any engine is touched."""
import numpy as np
import pytest

from fakebob_amd import query_eot as QE
from fakebob_amd.hsj import HopSkipJump
from fakebob_amd.kenansville import Kenansville
from fakebob_amd.pso import ParticleSwarm
from tests import vote_ref as V


def test_a_tie_between_two_speakers_goes_to_the_first():
    sc = np.array([[[0.5, 2.0, 2.0], [2.0, 0.5, 2.0], [0.1, 0.2, 3.0]]])        # one row, three replicas: decisions 1, 0, 2
    tv = np.ones((1, 3), np.int32)
    for task in ("OSI", "CSI"):
        assert V.vote(task, "targeted", 1, 0.0, sc, tv)[0].tolist() == [1]
        assert V.vote(task, "targeted", 0, 0.0, sc, tv)[0].tolist() == [1]
        assert V.vote(task, "targeted", 2, 0.0, sc, tv)[0].tolist() == [1]        # the tied speaker 2 wins no tie
        assert V.vote(task, "untargeted", 1, 0.0, sc, tv)[0].tolist() == [2]


def test_a_score_equal_to_the_threshold():
    thr = 1.25
    tv = np.ones((1, 2), np.int32)
    sv = np.array([[[thr], [np.nextafter(thr, -np.inf)]]])
    assert V.vote("SV", "targeted", 1, thr, sv, tv)[0].tolist() == [1]            # SV accepts at the threshold ...
    assert V.vote("SV", "untargeted", 1, thr, sv, tv)[0].tolist() == [1]          # ... and rejects one ulp below
    osi = np.array([[[0.0, thr], [0.0, np.nextafter(thr, -np.inf)]]])
    assert V.vote("OSI", "targeted", 1, thr, osi, tv)[0].tolist() == [1]          # OSI does not reject at the threshold
    assert V.vote("OSI", "targeted", -1, thr, osi, tv)[0].tolist() == [1]
    assert V.vote("CSI", "targeted", 1, thr, osi, tv)[0].tolist() == [2]          # CSI has no threshold


def test_replicas_without_voiced_frames_never_vote():
    sc = np.array([[[5.0, 1.0]] * 4, [[5.0, 1.0]] * 4])
    tv = np.array([[0, 0, 0, 0], [3, 0, -1, 7]], np.int32)
    for at, label in (("targeted", 0), ("untargeted", 1), ("untargeted", 0)):
        votes, nodec, mean = V.vote("CSI", at, label, 0.0, sc, tv)
        assert nodec.tolist() == [4, 2]
        assert votes[0] == 0                                                      # all replicas -2: vote 0, whatever the goal
        assert votes[1] == (2 if (at, label) != ("untargeted", 0) else 0)
        assert np.array_equal(mean, [[5.0, 1.0], [5.0, 1.0]])                      # the mean is over every replica's scores


def test_the_mean_adds_in_ascending_order():
    v = np.array([1e16, 1.0, -1e16, 1.0])
    _votes, _nodec, mean = V.vote("SV", "targeted", 1, 0.0, v.reshape(1, 4, 1), np.ones((1, 4), np.int32))
    assert mean[0, 0] == (((v[0] + v[1]) + v[2]) + v[3]) / 4.0 == 0.25


def test_the_majority_quorum():
    for r in range(1, 33):
        q = V.majority(r)
        assert q == QE.majority(r) == r // 2 + 1
        assert 2 * q > r and 2 * (q - 1) <= r                                     # the smallest strict majority
    assert V.flags([0, 2, 3, 4], V.majority(4)).tolist() == [False, False, True, True]


def test_quorum_codes():
    assert QE.quorum_code(None) == 0 and QE.quorum_code("majority") == -1 and QE.quorum_code(-1) == -1
    assert [QE.quorum_code(q) for q in (1, 7, 32)] == [1, 7, 32]
    for bad in (0, 33, -2, 1.5, "most", True):
        with pytest.raises(ValueError):
            QE.quorum_code(bad)


@pytest.mark.parametrize("cls", [ParticleSwarm, Kenansville, HopSkipJump])
def test_the_attack_classes_refuse_eot_without_a_quorum(cls):
    class Model(object):
        task = "OSI"
        engine = None
    with pytest.raises(ValueError, match="quorum"):
        cls("OSI", "targeted", Model(), eot_size=2)
    with pytest.raises(ValueError):
        cls("OSI", "targeted", Model(), eot_size=33, quorum="majority")
    with pytest.raises(ValueError):
        cls("OSI", "targeted", Model(), eot_size=2, quorum=33)
    a = cls("OSI", "targeted", Model(), eot_size=2, quorum="majority")
    assert (a.eot_size, a.quorum) == (2, "majority")
    b = cls("OSI", "targeted", Model(), eot_size=1)                               # one draw has a decision: no quorum needed
    assert (b.eot_size, b.quorum) == (1, None)
    c = cls("OSI", "targeted", Model())
    assert (c.eot_size, c.quorum) == (None, None)
    class Held(object):                                                          # an engine that already holds two companions
        eot, query_eot, companions = 2, None, np.zeros((2, 8), np.int16)
    assert QE.Settings(cls.__name__, Held(), None, "majority", None, 8, 16).replicas == 6       # they count: r' is the engine's
    assert QE.Settings(cls.__name__, Held(), 4, 3, [np.zeros(8)], 8, 16).replicas == 8         # companions= replace them
    assert QE.Settings(cls.__name__, Held(), None, None, None, 8, 16).replicas == 1            # the switch off: one query per row
    with pytest.raises(ValueError, match="quorum"):                              # companions without the switch: refused ...
        QE.Settings(cls.__name__, None, None, None, [np.zeros(8)], 8, 16)          # ... before an engine is read
