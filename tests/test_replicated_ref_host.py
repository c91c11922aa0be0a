"""tests/replicated_ref.py without a GPU: its averaging against a plain sequential float64 loop, its loss against the
oracle's loss_fn for every task and attack type, its row order on a hand-made 3 x 2 x 2 example, and the choice of inputs of
tests/test_gpu_replicated_batches.py -- every composed row of every case keeps voiced frames, judged by the oracle's front
end on the oracle's own NES rows.  (The normals of a noise stage come from a device hook; here a numpy generator stands in
for them: the VAD's count depends on the noise level, not on the draw, and the GPU test refuses a row without voiced frames
anyway.)"""
import numpy as np
import pytest

from fakebob_amd import input_transform as T
from tests import replicated_ref as RR


def test_averaging_is_sequential_float64_addition():
    rng = np.random.default_rng(5)
    for B, R_, S in ((3, 2, 1), (7, 5, 3), (4, 32, 8), (2, 1, 2)):
        rep_l = rng.normal(size=(B, R_)) * 10.0 ** rng.integers(-3, 8, size=(B, R_))     # magnitudes that make the order matter
        rep_sc = rng.normal(size=(B, R_, S)) * 10.0 ** rng.integers(-3, 8, size=(B, R_, S))
        loss, scores = RR.averages(rep_l, rep_sc)
        assert loss.shape == (B,) and scores.shape == (B, S)
        for b in range(B):
            acc = float(rep_l[b, 0])
            for rho in range(1, R_):
                acc = acc + float(rep_l[b, rho])
            assert loss[b] == acc / float(R_)
            for s in range(S):
                acc = float(rep_sc[b, 0, s])
                for rho in range(1, R_):
                    acc = acc + float(rep_sc[b, rho, s])
                assert scores[b, s] == acc / float(R_)
    v = np.array([[1e16, 1.0, -1e16, 1.0]])
    assert RR.averages(v, v[:, :, None])[0][0] == (((1e16 + 1.0) + -1e16) + 1.0) / 4.0 == 0.25      # not fsum's 0.5


@pytest.mark.parametrize("task,attack,S", [(t, a, S) for t, S in (("OSI", 3), ("CSI", 4), ("SV", 1))
                                           for a in ("targeted", "untargeted")])
def test_loss_is_the_oracles(oracle, task, attack, S):
    rng = np.random.default_rng(S)
    sc = rng.normal(size=(5, 4, S))
    d = dict(task=task, attack=attack, threshold=0.1, adver_thresh=0.05, target=min(1, S - 1), true=S - 1)
    got = RR.replica_losses(oracle, d, sc)
    assert got.shape == (5, 4)
    for b in range(5):
        for rho in range(4):
            want = oracle.loss(task, attack, sc[b, rho][None, :], threshold=0.1, adver_thresh=0.05, target=d["target"], true=d["true"])
            assert got[b, rho] == want[0]
    assert np.ptp(got) > 0.0


def test_row_order_on_a_hand_made_example():
    """B = 3, K = 2, eot = 2: sample 0 of every composed row names its (b, u) and the `normals` argument records (b, rho)"""
    B, K, r, n = 3, 2, 2, 4
    a0 = np.zeros(n, np.int16)
    q = np.stack([np.full(n, 100 * b, np.int16) for b in range(B)])
    comp = np.full((1, n), 1000, np.int16)
    seen = []

    def normals(b, rho, s):
        seen.append((b, rho, s))
        return np.full(n, float(rho), np.float32)           # noise:1 adds rho LSBs: the replica word shows in the sample
    rows = RR.composed_rows(q, a0, comp, T.parse("noise:1"), r, normals)
    assert rows.shape == (B, K, r, n)
    flat = rows.reshape(B * K * r, n)
    for b in range(B):
        for u in range(K):
            for j in range(r):
                row = RR.flat_row(b, u, j, K, r)
                assert row == b * K * r + u * r + j
                assert flat[row, 0] == 100 * b + 1000 * u + RR.replica_word(u, j, r)
    assert [int(w[0]) for w in flat] == [0, 1, 1002, 1003, 100, 101, 1102, 1103, 200, 201, 1202, 1203]
    assert seen == [(b, rho, 0) for b in range(B) for rho in range(K * r)]
    assert RR.flat_row(2, 1, 1, K, r) == 11 and RR.replica_word(1, 0, r) == 2

    class FirstSample(object):          # a scorer whose raw score is the row's first sample: raw_scores' order is the flat order
        def score_raw(self, lst):
            return np.array([[float(w[0])] for w in lst]), np.ones(len(lst), np.int32)
    raw, tv = RR.raw_scores(FirstSample(), rows, "score", None, 0, K, r)
    assert raw[:, 0].tolist() == [float(w[0]) for w in flat] and tv.shape == (B * K * r,)
    # swap_replicas exchanges whole rows of replicas and nothing else
    ref = dict(rep_l=np.arange(12.0).reshape(3, 4), rep_sc=np.arange(24.0).reshape(3, 4, 2))
    loss, scores = RR.swap_replicas(ref, 0, 2)
    assert loss.tolist() == [9.5, 5.5, 1.5] and scores[:, 0].tolist() == [19.0, 11.0, 3.0]
    assert ref["rep_l"][0, 0] == 0.0                        # (on copies)


@pytest.mark.parametrize("name", sorted(RR.CASES))
def test_every_composed_row_of_every_case_is_voiced(oracle, name):
    case = RR.CASES[name]
    audio, comp = RR.case_audio(case)
    p = RR.case_params(case)
    q = RR.host_nes_rows(oracle, case["spd"], p.sigma, RR.SEED, RR.STREAM, audio, RR.IT)
    B = 2 * (case["spd"] // 2) + 1
    assert q.shape == (B, case["n"]) and np.array_equal(q[0], RR.CP.cast_i16(audio))
    assert len({w.tobytes() for w in q}) == B               # the NES rows differ from one another
    rng = np.random.default_rng(1)
    tv = RR.host_voiced_counts(oracle, oracle.default_cfg(), q, comp, T.parse(case["chain"]), case["eot"],
                               lambda b, rho, s: rng.standard_normal(case["n"]).astype(np.float32))
    assert tv.shape == (case["rows"],)
    print("%s: voiced frames per row %d .. %d" % (name, tv.min(), tv.max()))
    assert tv.min() > 0
