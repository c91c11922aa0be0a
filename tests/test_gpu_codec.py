"""The telephone-line codec on the device (fb_set_codec; its contract is in include/fakebob_hip.h): k_codec against the numpy
restatement (tests/codec_ref.py, itself pinned to audioop by tests/test_codec_host.py) to the bit at the kernel's edges, its
position behind the chain -- and behind the air channel, the composition and the replication --, enrolment, attacks, the
clearing and the refusals, and the fenced library.  Samples, features, raw scores and statistics are compared with
np.array_equal; the two places where an NES batch's row meets a scoring call use the suite's bound for exactly that pair,
SCORE_TOL (tests/test_gpu_input_transform.py), because the two go through different kernels."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from fakebob_amd import _native, air_channel as A, companions as CP, input_transform as T
from fakebob_amd._native import FB_E_ARG, NativeError
from fakebob_amd.engine import Engine, nes_params, pso_params
from fakebob_amd.models import synthetic_audio, synthetic_ivector_system
from tests import air_channel_ref, codec_ref as R
from tests.companions_ref import compose_row, mean_over_replicas
from tests.input_transform_noise_ref import NOISE, ref_noisy
from tests.input_transform_ref import ref as chain_ref
from tests.test_gpu_input_transform import SCORE_TOL   # the bound between an NES batch's row and a scoring call

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "include", "fakebob_hip_test.h")) as _h:
    TILE = int(re.search(r"#define FB_CODEC_TILE (\d+)", _h.read()).group(1))   # the ADPCM kernel's LDS tile, in samples
N = 4000
SPD = 4
SEED, STREAM, EPOCH = 0x1234567887654321, 7, 3
ROOM = A.AirChannel(1000, 32, 3000.0, 0.995, 0.999)


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def golden():
    with np.load(os.path.join(ROOT, "tests", "golden", "codec_audioop.npz")) as z:
        return {k: z[k] for k in z.files}


def _rand(n, seed, amp=32767):
    return np.random.default_rng(seed).integers(-amp - 1, amp + 1, n).astype(np.int16)


def _audio(utt=9, n=N):
    return synthetic_audio(utt, n)


def _wav(utt=9, n=N):
    return CP.cast_i16(_audio(utt, n))


def _check(e, kind, rows):
    got = e.debug_codec(kind, rows)
    assert len(got) == len(rows)
    for b, (g, x) in enumerate(zip(got, rows)):
        want = R.codec(kind, x)
        assert g.dtype == np.int16 and g.shape == x.shape, (kind, b)
        assert np.array_equal(g, want), (kind, b, x.size, int(np.flatnonzero(g != want)[0]))


# ------------------------------------------------------------------------------------------- 1. kernel against reference
@pytest.mark.parametrize("kind", R.KINDS)
def test_all_values_and_the_golden_rows(eng, golden, kind):
    """one row of all 65 536 values (exhaustive for G.711; for ADPCM a ramp over 128 tiles), then audioop's rows -- the clamp
    row among them: the index at 0 and at 88, the predictor in both clips"""
    _check(eng, kind, [golden["all_values"]])
    rows = [golden["adpcm_in_" + n] for n in ("speech", "noise", "clamp")]
    _check(eng, kind, rows)
    if kind == "adpcm":
        got = eng.debug_codec(kind, rows)
        assert all(np.array_equal(g, golden["adpcm_out_" + n]) for g, n in zip(got, ("speech", "noise", "clamp")))
    else:
        assert np.array_equal(eng.debug_codec(kind, [golden["all_values"]])[0], golden[kind])


@pytest.mark.parametrize("kind", R.KINDS)
def test_row_lengths_around_the_tile(eng, kind):
    for i, n in enumerate((1, 2, 3, 63, 64, 65, TILE - 1, TILE, TILE + 1, 2 * TILE + 3)):
        _check(eng, kind, [_rand(n, 100 + i)])


@pytest.mark.parametrize("B", [1, 63, 64, 65, 130])
@pytest.mark.parametrize("kind", R.KINDS)
def test_batch_sizes(eng, kind, B):
    """rows of 70 and 71 samples by turns: every second row starts at an odd sample"""
    _check(eng, kind, [_rand(70 + (b & 1), 1000 + b, amp=32767 if b % 3 else 2000) for b in range(B)])


@pytest.mark.parametrize("kind", R.KINDS)
def test_mixed_lengths_with_odd_rows_first(eng, kind):
    """one workgroup's rows of very different lengths (a lane past its row's end idles), the odd lengths first so that later
    rows start misaligned; 20 rows: a second ADPCM workgroup, partly filled"""
    lens = [1, 65, TILE + 1, 7, 2 * TILE + 3, 2, TILE, 3 * TILE - 1, 64, 513, 1, 1, 4 * TILE, 9, TILE - 1, 33, 2 * TILE, 5, 1001, 8]
    rows = [_rand(n, 2000 + i) for i, n in enumerate(lens)]
    rows[4][:] = np.resize(R.clamp_row(), rows[4].size)      # the state's limits on a misaligned row across tile seams
    off = np.cumsum([0] + lens)
    assert any(o & 1 for o in off[:-1]) and any(not o & 1 for o in off[1:-1])
    _check(eng, kind, rows)


def test_the_hook_neither_reads_nor_changes_the_setting(eng):
    x = _rand(600, 5)
    eng.set_codec("ulaw")
    try:
        assert np.array_equal(eng.debug_codec("adpcm", [x])[0], R.adpcm(x))
        assert eng.codec == "ulaw"
        assert np.array_equal(eng.debug_input_transform([x])[0], x)          # the sample hooks ignore the codec
        assert np.array_equal(eng.debug_input_transform_eot([x], 2, SEED, STREAM, EPOCH)[0][1], x)
    finally:
        eng.set_codec(None)
    off = np.array([0, x.size], np.int64)
    for kind in (0, 4, -1):                                                  # the hook takes a codec, not "none"
        with pytest.raises(NativeError) as ex:
            _native.check(eng._L.fb_debug_codec(eng._h, ctypes.c_int(kind), _native.ptr(x), _native.ptr(off), ctypes.c_int(1),
                                                _native.ptr(np.empty_like(x))))
        assert ex.value.code == FB_E_ARG


# ---------------------------------------------------------------------------------------------------- 2. position
def _gmm(system, task="OSI"):
    ubm, spk = system
    e = Engine(0)
    if task == "SV":
        e.load_gmm([ubm, spk[0]])
    else:
        e.load_gmm([ubm] + spk)
    e.set_system(task)
    return e


def _iv():
    sy = synthetic_ivector_system(C=96, D=72, R=48, L=24, n_speakers=3, seed=11)
    e = Engine(0)
    e.load_ivector(sy, "OSI")
    return e


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("system", ["gmm", "ivector"])
def test_the_codec_sits_behind_the_chain(small_system, system, kind):
    """chain, then codec, then the front end: a plain engine fed codec_ref(chain_ref(x)) sees the same features and scores.
    (4001 samples: the second row starts at an odd sample; without a chain the codec reads the batch itself.)"""
    mk = (lambda: _gmm(small_system)) if system == "gmm" else _iv
    d, c = mk(), mk()
    try:
        wavs = [_wav(0, 4001), _wav(1, N), _wav(2, 3000)]
        d.set_codec(kind)
        for spec in ("qt:64,ms:3", None):
            chain = T.parse(spec)
            d.set_input_transform(chain)
            coded = [R.codec(kind, chain_ref(w, chain)) for w in wavs]
            assert not np.array_equal(coded[0], R.codec(kind, wavs[0])) or spec is None
            fd, Td = d.debug_feats(wavs[0])
            fc, Tc = c.debug_feats(coded[0])
            assert Td == Tc and fd.shape == fc.shape and np.array_equal(fd.view(np.uint32), fc.view(np.uint32)), spec
            assert np.array_equal(d.debug_mfcc(wavs[0]).view(np.uint32), c.debug_mfcc(coded[0]).view(np.uint32)), spec
            raw_d, tv_d = d.score_raw(wavs)
            raw_c, tv_c = c.score_raw(coded)
            assert np.array_equal(raw_d.view(np.uint64), raw_c.view(np.uint64)) and np.array_equal(tv_d, tv_c), spec
            raw_p, _ = c.score_raw(wavs)
            assert not np.array_equal(raw_p, raw_c)                           # the codec is what the front end reads
    finally:
        d.close()
        c.close()


# ----------------------------------------------------------------------- 3. air channel, EOT replicas and companions
def test_the_codec_behind_the_air_channel_the_composition_and_the_replicas(small_system):
    """K = 2, eot = 2, an air channel, at:20 (an SNR noise stage: its power is taken at the chain's input, the channel's
    output) and ADPCM on all four replicas of a row, each from the state (0, 0).  Row 0 of an NES batch is the clean audio, so
    its replicas are rebuilt on the host -- composition, room, chain, codec -- and scored on a plain engine; score0 and
    adver_loss of fb_get_grad must be their mean in the contract's order.  An NES batch's row and a scoring call agree to
    SCORE_TOL, the mean keeps that bound, and the OSI loss is a difference of two scores: 2 * SCORE_TOL
    (tests/test_gpu_air_channel.py, tests/test_gpu_companions.py)."""
    K, r, it, seed, stream = 2, 2, 4, 11, 6
    thr, adv_thr = 0.1, 0.05
    chain = T.parse("at:20")
    audio = _audio()
    comp = [_wav(20)]
    d, c = _gmm(small_system), _gmm(small_system)
    try:
        d.set_air_channel(ROOM)
        d.set_input_transform(chain)
        d.set_eot(r)
        d.set_companions(comp)
        d.set_codec("adpcm")
        p = nes_params("OSI", "targeted", samples_per_draw=SPD, threshold=thr, adver_thresh=adv_thr, seed=seed, stream=stream, target=1)
        fl, _g, al, sc0 = d.get_grad(p, audio, it=it)
        a0 = _wav()
        w = compose_row(a0, a0, np.stack(comp))                              # [K][N]: a_0 and the companion
        reps, uncoded = [], []
        for u in range(K):
            for j in range(r):
                rho = u * r + j
                taps, z, wd = d.debug_air_taps(seed, stream, it, 0, rho)
                assert np.array_equal(taps, air_channel_ref.taps(ROOM.taps, ROOM.predelay, ROOM.amp, ROOM.rho_lo, ROOM.rho_hi, z, wd))
                o = air_channel_ref.convolve(w[u], taps)
                normals = {s: d.debug_tf_noise(seed, stream, it, 0, rho, s, 0, o.size) for s, st in enumerate(chain) if st.kind == NOISE}
                uncoded.append(ref_noisy(o, chain, normals))
                reps.append(R.adpcm(uncoded[-1]))

        def mean_scores(rows):
            raw, tv = c.score_raw(rows)
            assert np.all(tv > 0)
            sc = c.system_scores(raw)                                        # [K * r][S]
            losses = (np.maximum(np.delete(sc, 1, axis=1).max(axis=1), thr) + adv_thr) - sc[:, 1]
            return mean_over_replicas(sc.T), float(mean_over_replicas(losses)), sc
        want_sc, want_al, sc = mean_scores(reps)
        plain_sc, _plain_al, _ = mean_scores(uncoded)
        stats = d.stats()
    finally:
        d.close()
        c.close()
    S = want_sc.size
    print("score0 %.3g adver_loss %.3g; the codec moves the mean score by %.3g" %
          (np.abs(sc0[:S] - want_sc).max(), abs(al - want_al), np.abs(plain_sc - want_sc).max()))
    assert np.abs(sc0[:S] - want_sc).max() <= SCORE_TOL
    assert abs(al - want_al) <= 2 * SCORE_TOL
    assert np.isfinite(fl)
    assert np.abs(plain_sc - want_sc).max() > 100 * SCORE_TOL                # without the codec the rows score elsewhere
    assert np.ptp(sc[:, 1]) > 10 * SCORE_TOL                                 # and the replicas do differ
    assert stats["scored_utts"] == (SPD + 1) * K * r                         # fb_stats counts what the front end scored


# ---------------------------------------------------------------------------------------------------- 4. enrolment
@pytest.mark.parametrize("kind", R.KINDS)
def test_enrolment_goes_through_the_line(small_system, kind):
    ubm, _spk = small_system
    d, c = Engine(0), Engine(0)
    try:
        for e in (d, c):
            e.load_gmm([ubm])
        d.set_codec(kind)
        w = _wav(5, 4001)
        occ_d, F_d, tv_d = d.gmm_acc_stats(w)
        occ_c, F_c, tv_c = c.gmm_acc_stats(R.codec(kind, w))
        occ_p, _F, _tv = c.gmm_acc_stats(w)
    finally:
        d.close()
        c.close()
    assert tv_d == tv_c > 0
    assert np.array_equal(occ_d.view(np.uint64), occ_c.view(np.uint64)) and np.array_equal(F_d.view(np.uint64), F_c.view(np.uint64))
    assert not np.array_equal(occ_d, occ_p)


# ------------------------------------------------------------------------------------------------------ 5. attacks
def _same(a, b):
    return a[1] == b[1] and all(np.array_equal(u, v) for u, v in zip(a, b) if isinstance(u, np.ndarray))


def test_an_attack_through_adpcm_is_reproducible_and_differs(small_system):
    p = nes_params("OSI", "targeted", samples_per_draw=SPD, max_iter=5, target=1, epsilon=0.002, threshold=1e3, seed=5, stream=2)
    runs = []
    for codec in ("adpcm", "adpcm", None):
        e = _gmm(small_system)
        try:
            e.set_codec(codec)
            runs.append(e.attack(p, _audio()))
        finally:
            e.close()
    assert runs[0][3].shape[0] == 5 and np.all(np.isfinite(runs[0][3]))
    assert _same(runs[0], runs[1])                                           # a fresh engine, the same seed
    assert not np.array_equal(runs[0][3], runs[2][3])                        # and the line is not transparent


def test_the_returned_audio_is_raw(small_system):
    """SV, a threshold just above the clean score through the line, so the attack stops with success after at least one
    step and its last trace row holds the scores of the audio it returns.  That audio is the attacker's, not the line's
    output: it stays in the epsilon ball around the input, it is the cast of the float audio, and scoring it through the same
    engine -- a scoring call against the NES batch's row 0: SCORE_TOL -- gives the last trace row."""
    audio = _audio()
    d = _gmm(small_system, "SV")
    try:
        d.set_codec("adpcm")
        raw, _ = d.score_raw([_wav()])
        s0 = float(d.system_scores(raw)[0, 0])
        p = nes_params("SV", "targeted", samples_per_draw=20, max_iter=60, epsilon=0.002, threshold=s0 + 0.005, seed=1, stream=0)
        adv, flag, adv_f, trace = d.attack(p, audio)
        raw_a, _ = d.score_raw([adv])
        sc_a = d.system_scores(raw_a)[0]
        d.set_codec(None)
        raw_p, _ = d.score_raw([adv])
        sc_p = d.system_scores(raw_p)[0]
    finally:
        d.close()
    print("flag %d after %d iterations; |last trace row - rescored| %.3g; without the line %.3g" %
          (flag, trace.shape[0], np.abs(trace[-1, 3:] - sc_a).max(), np.abs(trace[-1, 3:] - sc_p).max()))
    assert flag == 1 and trace.shape[0] >= 2, "the attack through the line did not succeed within 60 iterations"
    assert abs(trace[0, 3] - s0) <= SCORE_TOL
    assert np.abs(adv_f - audio).max() <= 0.002 + 1e-15
    assert np.array_equal(adv, np.trunc(adv_f * 32768.0).astype(np.int64).astype(np.int16))
    assert not np.array_equal(adv, R.adpcm(adv))
    assert np.all(trace[:, 0] <= 0.002 + 1e-12) and trace[-1, 0] > 0          # the distance column is the raw audio's too
    assert np.abs(trace[-1, 3:] - sc_a).max() <= SCORE_TOL
    assert np.abs(trace[-1, 3:] - sc_p).max() > 100 * SCORE_TOL


def test_the_swarm_flies_through_the_line(small_system):
    """particle 0 of the first iteration is the original audio: its loss through mu-law is the loss of the host-coded audio
    on an engine without a codec (the same kernels over the same samples)"""
    audio = _audio()
    d, c = _gmm(small_system), _gmm(small_system)
    try:
        d.set_codec("ulaw")
        p = nes_params("OSI", "targeted", epsilon=0.002, max_iter=3, target=1, threshold=1e3, seed=5, stream=1)
        q = pso_params(particles=4)
        through = d.attack_pso(p, q, audio)
        coded = R.ulaw(_wav())
        plain = c.attack_pso(p, q, coded.astype(np.float64) / 32768.0)
        raw = c.attack_pso(p, q, audio)
    finally:
        d.close()
        c.close()
    assert through[4].shape == (3, 4) and np.all(np.isfinite(through[4]))
    assert through[4][0][0] == plain[4][0][0]
    assert through[4][0][0] != raw[4][0][0]
    assert np.abs(through[2] - audio).max() <= 0.002 + 1e-15                 # the returned audio is not coded


# ------------------------------------------------------------------------------------------------ 6. off means off
@pytest.mark.parametrize("system", ["gmm", "ivector"])
def test_off_means_off_and_refusals_keep_the_setting(small_system, system):
    mk = (lambda: _gmm(small_system)) if system == "gmm" else _iv
    d, c = mk(), mk()
    try:
        wavs = [_wav(0, 4001), _wav(1)]
        base, tv = c.score_raw(wavs)
        for kind in R.KINDS:
            d.set_codec(kind)
            coded, _ = d.score_raw(wavs)
            assert not np.array_equal(coded, base), kind
            for bad in (4, -1):
                with pytest.raises(NativeError) as ex:
                    d.set_codec(bad, validate=False)                         # past the wrapper: the library's own refusal
                assert ex.value.code == FB_E_ARG
                assert d.codec == kind
                again, _ = d.score_raw(wavs)
                assert np.array_equal(again.view(np.uint64), coded.view(np.uint64)), (kind, bad)   # the previous codec is in force
            with pytest.raises(ValueError):
                d.set_codec("gsm")                                           # the wrapper's
            d.set_codec("none" if kind == "alaw" else None)
            assert d.codec is None
            off, tv_off = d.score_raw(wavs)
            assert np.array_equal(off.view(np.uint64), base.view(np.uint64)) and np.array_equal(tv_off, tv), kind
    finally:
        d.close()
        c.close()


# ------------------------------------------------------------------------------------------------ 7. fenced library
CHILD = r'''
import sys
import numpy as np
sys.path.insert(0, %(root)r)
from fakebob_amd.engine import Engine, nes_params
from fakebob_amd.models import synthetic_audio, synthetic_gmm_system
out = {}
rng = np.random.default_rng(3)
rows = [rng.integers(-32768, 32768, n).astype(np.int16) for n in (1, 65, 513, 7, 1027, 4000)]
ubm, spk = synthetic_gmm_system(n_speakers=3, C=256, D=72)
e = Engine(0)
e.load_gmm([ubm] + spk)
e.set_system("OSI")
for kind in ("ulaw", "alaw", "adpcm"):
    out["rows_" + kind] = np.concatenate(e.debug_codec(kind, rows))
e.set_input_transform("qt:64,ms:3")
e.set_codec("adpcm")
p = nes_params("OSI", "targeted", samples_per_draw=4, max_iter=5, target=1, epsilon=0.002, threshold=1e3, seed=5, stream=2)
adv, flag, advf, trace = e.attack(p, synthetic_audio(9, 4000))
out["trace"] = np.asarray(trace).copy()
out["adv"] = np.asarray(advf)
e.close()
np.savez(sys.argv[1], **out)
'''


def test_fenced_build_gives_the_same_bits(tmp_path):
    """codec_kernel.hip exchanges nothing between workgroups, so the fenced library links the product build's object: the same
    rows and the same attack through the line from either library"""
    from fakebob_amd import build
    lib, fenced = build.LIB, build.variant_path("fenced")
    assert os.path.exists(fenced), "libfakebob_hip_fenced.so not built (__graft_entry__.build() builds it)"
    res = []
    for name, path in (("plain", lib), ("fenced", fenced)):
        out = str(tmp_path / (name + ".npz"))
        r = subprocess.run([sys.executable, "-c", CHILD % {"root": ROOT}, out], env=dict(os.environ, FAKEBOB_HIP_LIB=path),
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-3000:]
        res.append(np.load(out))
    a, b = res
    assert sorted(a.files) == sorted(b.files)
    for k in a.files:
        x, y = a[k], b[k]
        assert x.shape == y.shape and np.array_equal(x.view(np.uint64) if x.dtype == np.float64 else x,
                                                     y.view(np.uint64) if y.dtype == np.float64 else y), k
    assert a["trace"].shape[0] == 5
