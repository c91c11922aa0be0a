"""White-box gradients under a play offset on the device (fb_set_play_offset with fb_set_wb_universal; the "Transposed rule" of
the "Play offset" section of include/fakebob_hip.h).

Exact: k_wb_play_compose_t alone against the numpy sum of tests/play_offset_ref.py (the hook), and the launch counts.
One comparison carries a bar: fb_get_grad_wb_from against PyTorch float64 autograd over tests/play_offset_vjp_ref.py's function,
as a relative L2 error ||g - g_ref|| / ||g_ref||.  The offset only permutes indices, so the yardstick is the universal path's own
agreement in the same test process, on the same system and inputs at S = 0: the offset case must lie within 4 x that value (the
summation order over the R terms is unchanged; 4 x covers a different set of clipped samples).  Both values are printed."""
import numpy as np
import pytest

from fakebob_amd import air_channel as A
from fakebob_amd import input_transform as IT
from fakebob_amd.engine import Engine, nes_params
from fakebob_amd.models import synthetic_ivector_system
from tests import play_offset_ref as R
from tests import play_offset_vjp_ref as PV
from tests import universal_vjp_ref as U
from tests import whitebox_iv_ref as V
from tests.test_gpu_whitebox import _load, rel_l2
from tests.test_universal_vjp_host import _rail_case

pytestmark = pytest.mark.gpu

SEED, STREAM, IT_ = 77, 3, 5
N = 4000
ROOM64 = A.AirChannel(64, 8, 3000.0, 0.9, 0.99)
IV_SMALL = dict(C=64, D=72, R=32, L=16, n_speakers=2, seed=4)
OSI_KW = dict(target=1, threshold=-10.0)


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


def _clear(e):
    e.set_play_offset(0)
    e.set_air_channel(None)
    e.set_input_transform(None)
    e.set_companions(None)
    e.set_eot(1)
    e.set_wb_bpda(False)
    e.set_wb_ivector(False)
    e.set_wb_air(False)
    e.set_wb_universal(False)


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


# ------------------------------------------------------------------------------------- 1. the hook, exactly
@pytest.mark.parametrize("K,eot", [(1, 1), (3, 1), (4, 8)])
@pytest.mark.parametrize("n", [1, 2, 257, 4001])
def test_hook_play_compose_t_is_the_numpy_sum(eng, K, eot, n):
    rng = np.random.RandomState(1000 * K + n)
    q, a0, comp3 = _rail_case(n, n + K)
    comp = comp3[rng.randint(0, 3, K - 1)] if K > 1 else None
    Rn = K * eot
    tau = rng.randint(0, n, Rn)
    tau[0] = 0
    tau[-1] = n - 1
    if Rn > 2:
        tau[1] = n // 2
    if K > 1 and n > 2:                                      # clipped samples on both sides of the last replica's wrap
        d = q.astype(np.int32) - a0.astype(np.int32)
        for i in (n - 2, n - 1, 0):                          # composed sample i of replica Rn - 1 takes d[(i - tau) mod n]
            k = (i - int(tau[-1])) % n
            comp[-1, i] = 32767 if d[k] > 0 else -32768
            if d[k] == 0:
                q[k] += 1
                comp[-1, i] = 32767
    if K > 1 and n >= 257:                                   # ... and samples exactly AT a rail, not clipped, under that offset
        k5, k6 = (5 - int(tau[-1])) % n, (6 - int(tau[-1])) % n
        q[k5], q[k6] = a0[k5] + 7, a0[k6] - 7                # d = +7 and -7 there
        comp[-1, 5], comp[-1, 6] = 32767 - 7, -32768 + 7
    cots = rng.randint(-2 ** 20, 2 ** 20, (Rn, n)).astype(np.float64) + rng.rand(Rn, n)      # (roundings in the sum do happen)
    got = eng.debug_wb_play_compose_t(cots, q, a0, comp, tau, eot)
    assert eng.debug_wb_play_route() == 1
    want = R.compose_t(cots, q, a0, comp, eot, tau)
    assert np.array_equal(_bits(got), _bits(want)), (K, eot, n)
    m = R.mask(q, a0, comp, eot, tau)
    if K > 1 and n > 2:
        assert not m[-1, [n - 2, n - 1, 0]].any()            # ... and they are masked
    if K > 1 and n >= 257:
        rows = R.compose_rows(q, a0, comp, eot, tau)
        assert (~m).any() and m[-1, 5] and m[-1, 6] and rows[-1, 5] == 32767 and rows[-1, 6] == -32768   # at a rail, unclipped: passes
    zero = eng.debug_wb_play_compose_t(np.zeros((Rn, n)), q, a0, comp, tau, eot)
    assert np.array_equal(_bits(zero), _bits(np.zeros(n)))   # +0.0 everywhere
    if n > 1:
        same = eng.debug_wb_play_compose_t(cots, q, a0, comp, np.zeros(Rn, np.uint32), eot)  # tau = 0, K = 1: the plain sum
        if K == 1:
            acc = np.zeros(n)
            for rho in range(Rn):
                acc = acc + cots[rho]
            assert np.array_equal(_bits(same), _bits(acc))


# ------------------------------------------------------------------------------------- 2. the whole gradient
def _chain(spec):
    return [tuple(s) for s in IT.parse(spec)] if spec else []


def _setup(e, comp, spec, air, ivector, S):
    e.set_input_transform(spec)
    e.set_air_channel(ROOM64 if air else None)
    e.set_eot(1)
    e.set_companions(comp)
    e.set_wb_bpda(bool(spec))
    e.set_wb_air(bool(air))
    e.set_wb_ivector(bool(ivector))
    e.set_wb_universal(True)
    e.set_play_offset(S)


CASES = [(v, spec, air) for v in ("gmm", "ivector") for spec in (None, "ms:3") for air in (False, True)]


@pytest.mark.parametrize("victim,spec,air", CASES, ids=["%s-%s-%s" % (v, s or "plain", "air64" if a else "noair") for v, s, a in CASES])
def test_get_grad_wb_from_against_autograd(eng, small_system, victim, spec, air):
    """K = 2 (one loud companion: part of its samples clip), eot = 1, S = N - 1 against S = 0"""
    audio, original, comp = U.perturbed_case(N, 1)
    iv = victim == "ivector"
    if iv:
        sy = synthetic_ivector_system(**IV_SMALL)
        tab = V.IvTables(sy)
        eng.load_ivector(sy, "OSI")
        models = None
    else:
        models = _load(eng, small_system, "OSI")
    p = nes_params("OSI", "targeted", samples_per_draw=0, seed=SEED, stream=STREAM, **OSI_KW)
    chain, Rn = _chain(spec), 2
    out = {}
    try:
        for S in (0, N - 1):
            _setup(eng, comp, spec, air, iv, S)
            grad, al, sc = eng.get_grad_wb_from(p, audio, original, IT_)
            uni, play = eng.debug_wb_universal_route(), eng.debug_wb_play_route()
            sel = eng.debug_iv_gselect()[0] if iv else None
            tau = eng.debug_play_offsets(SEED, STREAM, IT_, 1, Rn)[0] if S else None
            taps = [eng.debug_air_taps(SEED, STREAM, IT_, 0, rho)[0] for rho in range(Rn)] if air else None
            out[S] = (grad, al, sc, uni, play, sel, tau, taps)
    finally:
        _clear(eng)
        if iv:
            _load(eng, small_system, "OSI")
    err, refs = {}, {}
    for S, (grad, al, sc, uni, play, sel, tau, taps) in out.items():
        kw = dict(r=1, tau=tau, chain=chain, taps=taps, **OSI_KW)
        if iv:
            own = PV.loss_and_grad_iv(eng.cfg, tab, "OSI", "targeted", audio, original, comp, **kw)
            assert sel.shape[0] == sum(own.tv)
            cuts = np.cumsum([0] + own.tv)
            ref = PV.loss_and_grad_iv(eng.cfg, tab, "OSI", "targeted", audio, original, comp, sels=[sel[cuts[i]:cuts[i + 1]] for i in range(Rn)], **kw)
        else:
            ref = PV.loss_and_grad(eng.cfg, models, "OSI", "targeted", audio, original, comp, **kw)
        err[S], refs[S] = rel_l2(grad, ref.grad), ref
        print("%s %s %s S = %d: tau %s, Tv %s, loss %.9g (restatement %.9g), VAD margin %.3g, relative L2 error %.3g"
              % (victim, spec, air, S, None if tau is None else tau.tolist(), ref.tv, al, ref.loss, ref.margin, err[S]))
        assert (uni, play) == ((1, 0) if S == 0 else (0, 1))           # one launch of the one kernel, none of the other
        assert np.isfinite(grad).all() and grad.any()
        assert abs(al - ref.loss) < 1e-3 and np.abs(sc[:ref.scores.size] - ref.scores).max() < 1e-3
    tau = out[N - 1][6]
    assert tau[0] != tau[1] and tau.max() > 0                           # the replicas do hear different offsets
    want_rows = R.compose_rows(U.quantize(audio), U.quantize(original), comp, 1, tau)
    assert np.array_equal(refs[N - 1].rows, want_rows)                  # the autograd function composes what the contract says
    assert not R.mask(U.quantize(audio), U.quantize(original), comp, 1, tau).all()           # and the clip is exercised
    assert not np.array_equal(out[0][0], out[N - 1][0])
    assert refs[0].margin > 1e-3 and refs[N - 1].margin > 1e-3
    assert err[N - 1] <= 4.0 * err[0], (err[N - 1], err[0])


# ------------------------------------------------------------------------------------- 3. the route of an attack
def test_an_attack_launches_one_transposed_composition_per_iteration(eng, small_system):
    audio, comp = U.utterances(N, 1)
    _load(eng, small_system, "OSI")
    p = nes_params("OSI", "targeted", target=1, threshold=1e3, max_iter=3, seed=SEED, stream=STREAM)
    try:
        counts = {}
        for K1 in (0, 1):
            for S in (0, 500):
                _setup(eng, comp if K1 else None, None, False, False, S)
                res = eng.attack_wb(p, audio)
                assert res[3].shape[0] == 3
                counts[(K1, S)] = (eng.debug_wb_universal_route(), eng.debug_wb_play_route(), eng.debug_play_route())
                again = eng.attack_wb(p, audio)
                assert all(np.array_equal(x, y) for x, y in zip(res, again))      # the same bits on every run
        eng.set_play_offset(500)
        g1 = eng.get_grad_wb_from(p, audio + 3.0 / 32768.0, audio, 2)
        g2 = eng.get_grad_wb_from(p, audio + 3.0 / 32768.0, audio, 2)
        assert np.array_equal(_bits(g1[0]), _bits(g2[0])) and g1[1] == g2[1]
    finally:
        _clear(eng)
    assert counts[(0, 0)] == (0, 0, 0) and counts[(1, 0)] == (3, 0, 0)              # S = 0: k_wb_compose_t with companions only
    assert counts[(0, 500)][:2] == (0, 3) and counts[(1, 500)][:2] == (0, 3)        # S > 0: k_wb_play_compose_t, also at K = 1
    assert counts[(0, 500)][2] == 3 and counts[(1, 500)][2] == 3                    # (k_play_compose: one per forward)
