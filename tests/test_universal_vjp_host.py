"""The restatement of the white-box gradient of a universal perturbation (tests/universal_vjp_ref.py) on the CPU: its composition
against tests/companions_ref.compose_row, the composition's transpose against the adjoint identity, autograd against central
differences at a point where no composed sample is within 1 of a rail, K = 1 against tests/whitebox_ref.py, and the inputs of the
attack comparison that tests/test_gpu_wb_universal.py repeats on the device; and the driver's rules for --wb-universal on the stub
site of tests/golden/driver_site.py.

Bars: the composition is integer arithmetic (exact); with integer-valued cotangents the adjoint identity is exact, with normal
ones it holds to float64 summation error (1e-12 relative); differences against autograd as tests/test_whitebox_ref_host.py:
1e-6 relative; K = 1 is the same graph: equal bits."""
import numpy as np
import pytest
import torch

from fakebob_amd.models import stack_models
from tests import universal_vjp_ref as U
from tests import whitebox_ref as R
from tests.companions_ref import compose_row
from tests.test_feco_vjp_host import _directional
from tests.test_whitebox_host import _main, site      # noqa: F401 (site is a fixture)

OSI_KW = dict(target=1, threshold=-10.0)

# the attack comparison (here and on the device): SV, a threshold no score reaches, thirty plain sign steps of ATTACK_LR inside
# the default epsilon ball, K = 4 utterances of 4000 samples: universal_vjp_ref.utterances(4000, 3)
ATTACK_N, ATTACK_K1, ATTACK_STEPS, ATTACK_LR, ATTACK_EPS, ATTACK_THRESHOLD = 4000, 3, 30, 0.0005, 0.002, 1e3


def _stack(small_system, task):
    ubm, spk = small_system
    return stack_models(spk if task == "CSI" else ([ubm] + spk if task == "OSI" else [ubm, spk[0]]))


def _rail_case(n, seed):
    """q, a0 and three companions with samples that clip at either rail, samples exactly AT a rail unclipped, and the rest inside"""
    rng = np.random.RandomState(seed)
    q = rng.randint(-3000, 3000, n).astype(np.int16)
    a0 = (q.astype(np.int32) - rng.randint(-40, 41, n)).astype(np.int16)
    d = q.astype(np.int32) - a0.astype(np.int32)
    comp = rng.randint(-32768, 32768, (3, n)).astype(np.int32)
    kind = rng.randint(0, 6, (3, n))
    comp = np.where(kind == 0, 32767 - d, comp)              # AT the upper rail, not clipped
    comp = np.where(kind == 1, -32768 - d, comp)             # AT the lower rail, not clipped
    comp = np.where(kind == 2, 32767 - d + 1, comp)          # one past the upper rail
    comp = np.where(kind == 3, -32768 - d - 1, comp)         # one past the lower rail
    return q, a0, np.clip(comp, -32768, 32767).astype(np.int16)


def test_the_composition_is_companions_refs():
    for n, seed in ((1, 1), (257, 2), (4000, 3)):
        q, a0, comp = _rail_case(n, seed)
        rows = U.compose(torch.tensor(q.astype(np.float64)), a0, comp)
        got = np.stack([w.numpy() for w in rows])
        want = compose_row(q, a0, comp)
        assert np.array_equal(got, want.astype(np.float64))
        m = U.mask_rows(q, a0, comp)
        v = comp.astype(np.int64) + q.astype(np.int64) - a0.astype(np.int64)
        assert m[0].all() and np.array_equal(m[1:], (v >= -32768) & (v <= 32767))
        if n >= 257:
            assert (~m[1:]).any() and (m[1:] & ((want[1:] == 32767) | (want[1:] == -32768))).any()    # clipped, and AT a rail unclipped


def test_the_transpose_is_the_adjoint_of_the_composition():
    q, a0, comp = _rail_case(4000, 4)
    rng = np.random.default_rng(5)
    for r in (1, 2):
        for integer in (True, False):
            cots = rng.integers(-1000, 1000, (4 * r, 4000)).astype(np.float64) if integer else rng.normal(size=(4 * r, 4000))
            dq = rng.integers(-5, 6, 4000).astype(np.float64) if integer else rng.normal(size=4000)
            g = U.compose_t(cots, q, a0, comp, r)
            x = torch.tensor(q.astype(np.float64), requires_grad=True)
            rows = U.compose(x, a0, comp)
            sum((rows[rho // r] * torch.as_tensor(cots[rho])).sum() for rho in range(4 * r)).backward()
            auto = x.grad.numpy()
            # <cots, J dq> with J the composition's Jacobian under the mask rule, row by row
            m = U.mask_rows(q, a0, comp)
            lhs = sum(float(np.dot(cots[rho], np.where(m[rho // r], dq, 0.0))) for rho in range(4 * r))
            rhs = float(np.dot(g, dq))
            if integer:
                assert np.array_equal(g, auto) and lhs == rhs
            else:
                assert np.abs(g - auto).max() <= 1e-12 * np.abs(auto).max() and abs(lhs - rhs) <= 1e-12 * abs(lhs)
            masked = ~m[1:].any(axis=0)
            assert masked.any() and np.array_equal(g[masked], (cots[0] if r == 1 else cots[0] + cots[1])[masked])     # utterance 0 intact


def test_gradient_against_central_differences_away_from_the_rails(oracle, small_system):
    cfg = oracle.default_cfg()
    models = _stack(small_system, "OSI")
    audio, original, comp = U.perturbed_case(4000, 2)
    v = comp.astype(np.int64) + (U.quantize(audio).astype(np.int64) - U.quantize(original).astype(np.int64))
    near = (np.abs(v - 32767) <= 1) | (np.abs(v + 32768) <= 1)
    comp = np.where(near, comp // 2, comp).astype(np.int16)          # (no sample within 1 of a rail: the mask cannot flip under h)
    v = comp.astype(np.int64) + (U.quantize(audio).astype(np.int64) - U.quantize(original).astype(np.int64))
    assert not ((np.abs(v - 32767) <= 1) | (np.abs(v + 32768) <= 1)).any()
    r = U.loss_and_grad(cfg, models, "OSI", "targeted", audio, original, comp, cast=False, **OSI_KW)
    print("K = 3: loss %.9g, losses %s, clipped %s, min |c0 - thr| %.3g" % (r.loss, r.losses, r.clipped, r.margin))
    assert r.margin > 1e-3 and r.clipped[0] == 0 and r.clipped[1] >= 40 and r.clipped[2] == 0

    def f(a):
        return U.loss_and_grad(cfg, models, "OSI", "targeted", a, original, comp, cast=False, **OSI_KW).loss
    assert _directional(f, r.grad, audio) < 1e-6


def test_one_utterance_is_whitebox_refs_gradient(oracle, small_system):
    cfg = oracle.default_cfg()
    audio = R.test_audio(4000)
    for task, attack, kw in (("OSI", "targeted", OSI_KW), ("SV", "untargeted", dict(threshold=0.1))):
        models = _stack(small_system, task)
        want = R.loss_and_grad(cfg, models, task, attack, audio, **kw)
        got = U.loss_and_grad(cfg, models, task, attack, audio, **kw)
        assert got.loss == want.loss and np.array_equal(got.grad, want.grad) and np.array_equal(got.scores, want.scores)
        got = U.loss_and_grad(cfg, models, task, attack, audio, original=R.test_audio(4000) * 0.5, **kw)      # a_0 is not read at K = 1
        assert got.loss == want.loss and np.array_equal(got.grad, want.grad)


def test_one_utterance_on_the_ivector_victim_is_whitebox_iv_refs_gradient(oracle):
    from fakebob_amd.models import synthetic_ivector_system
    from tests import whitebox_iv_ref as V
    cfg = oracle.default_cfg()
    tab = V.IvTables(synthetic_ivector_system(C=64, D=72, R=32, L=16, n_speakers=2, seed=4))
    audio = R.test_audio(4000)
    want = V.loss_and_grad_iv(cfg, tab, "OSI", "targeted", audio, **OSI_KW)
    got = U.loss_and_grad_iv(cfg, tab, "OSI", "targeted", audio, **OSI_KW)
    assert got.loss == want.loss and np.array_equal(got.grad, want.grad) and np.array_equal(got.scores, want.scores)
    # the GPU cases' preconditions hold in the restatement: VAD and pruning margins, the share of clear selections
    audio, original, comp = U.perturbed_case(4000, 3)
    r = U.loss_and_grad_iv(cfg, tab, "OSI", "targeted", audio, original, comp, **OSI_KW)
    assert r.margin > 1e-3 and r.clipped[1] >= 40
    assert all(ex.prune_margin >= 1e-5 and (ex.gsel_gap >= 1e-3).mean() >= 0.9 for ex in r.reps)


def attack_comparison(cfg, models):
    """-> (clean, universal, single): the mean loss over the K utterances before the steps, after the steps on the gradient of the
    mean, and after the same steps on utterance 0's gradient alone, all in the restatement"""
    audio, comp = U.utterances(ATTACK_N, ATTACK_K1)
    kw = dict(threshold=ATTACK_THRESHOLD)

    def mean_loss(a):
        r = U.loss_and_grad(cfg, models, "SV", "untargeted", a, audio, comp, **kw)
        assert r.margin > 1e-3
        return r.loss
    uni = U.sign_steps(cfg, models, "SV", "untargeted", audio, comp, ATTACK_STEPS, ATTACK_LR, ATTACK_EPS, True, **kw)
    one = U.sign_steps(cfg, models, "SV", "untargeted", audio, comp, ATTACK_STEPS, ATTACK_LR, ATTACK_EPS, False, **kw)
    return mean_loss(audio), mean_loss(uni), mean_loss(one)


def test_the_universal_steps_beat_the_single_utterance_steps(oracle, small_system):
    clean, universal, single = attack_comparison(oracle.default_cfg(), _stack(small_system, "SV"))
    print("mean loss over K = %d utterances: clean %.9g, universal %.9g, utterance 0's steps %.9g" % (ATTACK_K1 + 1, clean, universal, single))
    assert universal < clean and universal < single      # (float64 on the CPU: 1000.03685 / 999.214802 / 999.669118)


# ------------------------------------------------------------------------------------------------ attack_main's rules
def test_attack_main_hands_pgd_the_universal_option(site):
    _res, seen = _main(["--attack", "pgd", "--wb-universal", "-max_iter", "4"])
    assert seen[0]["universal"] is True and seen[0]["bpda"] is False and "eot_size" not in seen[0]
    _res, seen = _main(["--attack", "pgd", "--wb-universal", "--bpda", "--eot-size", "2", "-max_iter", "4"])
    assert seen[0]["universal"] is True and seen[0]["bpda"] is True and seen[0]["eot_size"] == 2
    _res, seen = _main(["--attack", "pgd", "-archi", "iv", "--wb-ivector", "--wb-universal", "--bpda", "--eot-size", "2", "-max_iter", "4"])
    assert seen[0]["universal"] is True and seen[0]["bpda"] is True and seen[0]["eot_size"] == 2       # IvectorPGD's eot_size
    _res, seen = _main(["--attack", "pgd", "-archi", "iv", "--wb-ivector", "--wb-universal", "-max_iter", "4"])
    assert seen[0]["universal"] is True and "bpda" not in seen[0] and "eot_size" not in seen[0]


@pytest.mark.parametrize("extra", [["--attack", "nes", "--wb-universal"], ["--wb-universal"], ["--attack", "pso", "--wb-universal"],
                                   ["--attack", "pgd", "--companions", "1"],                               # without the flag: as before
                                   ["--attack", "pgd", "--wb-universal", "--eot-size", "2"],               # EOT still needs --bpda
                                   ["--attack", "pgd", "-archi", "iv", "--wb-universal"],                  # -archi iv still needs --wb-ivector
                                   ["--attack", "pgd", "--wb-universal", "--companions", "1", "--feco", "0.5"]])
def test_attack_main_refuses_before_any_model_is_built(site, extra):
    built = []
    with pytest.raises(SystemExit):
        _main(extra, built)
    assert built == []
