"""A numpy restatement of the voted decision (fb_set_query_eot; the "voted decisions" section of include/fakebob_hip.h): the
system scores of every replica row, its decision and flag by the decision-only attacks' rule, the row's vote, the replicas
without a decision, and fb_set_eot's mean of the replicas' score rows.  Every value is float64 arithmetic with one rounding per
operation, so the device launch (k_vote) is compared bit for bit."""
import numpy as np

from tests.input_transform_noise_ref import eot_mean
from tests.kenansville_ref import decide, succeeds


def majority(replicas):
    """the majority quorum of r' replicas"""
    return int(replicas) // 2 + 1


def system_scores(task, raw, z_mean=None, z_std=None, znorm_all=False):
    """raw (..., M) -> the system scores (..., S): z-normalised (CSI, or every i-vector system) or against the UBM in column 0"""
    raw = np.asarray(raw, np.float64)
    if task == "CSI" or znorm_all:
        return (raw - np.asarray(z_mean, np.float64)) / np.asarray(z_std, np.float64)
    return raw[..., 1:] - raw[..., :1]


def vote(task, attack_type, label, threshold, scores, tv):
    """scores (rows, r', S) and tv (rows, r') -> votes (rows,) int32: the adversarial replicas of every row; nodec (rows,)
    int32: its replicas without voiced frames; mean (rows, S): the replicas' scores averaged, rho ascending"""
    scores = np.asarray(scores, np.float64)
    rows, r, S = scores.shape
    tv = np.asarray(tv).reshape(rows, r)
    votes, nodec = np.zeros(rows, np.int32), np.zeros(rows, np.int32)
    for b in range(rows):
        for j in range(r):
            d = decide(task, scores[b, j], threshold, tv[b, j])
            nodec[b] += d == -2
            votes[b] += bool(succeeds(d, attack_type, label))
    return votes, nodec, eot_mean(scores.transpose(0, 2, 1))


def flags(votes, quorum):
    """which rows are voted adversarial"""
    return np.asarray(votes) >= int(quorum)
