"""FB_TF_NOISE on the device (include/fakebob_hip.h: the stage contract and the "Noise RNG contract"): the transform
kernel against the numpy restatement fed the generator's own normals, bit for bit; the normals themselves; scoring through a
noise chain; the refusals."""
import numpy as np
import pytest

from fakebob_amd import input_transform as T
from fakebob_amd._native import FB_E_ARG, NativeError
from fakebob_amd.engine import Engine
from fakebob_amd.models import synthetic_audio, synthetic_ivector_system
from tests.input_transform_noise_ref import NOISE, ref_noisy

pytestmark = pytest.mark.gpu
TILE = 4096
SEED, STREAM, EPOCH = 0x1234567887654321, 7, 3
LENGTHS = [1, 5, TILE - 1, TILE, TILE + 1, 3 * TILE + 17]


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


def _rand(n, seed, amp=3000):
    return np.random.default_rng(seed).integers(-amp, amp + 1, n).astype(np.int16)


def _want(eng, w, chain, utt, replica, seed=SEED, stream=STREAM, epoch=EPOCH):
    normals = {s: eng.debug_tf_noise(seed, stream, epoch, utt, replica, s, 0, w.size)
               for s, st in enumerate(chain) if st.kind == NOISE}
    return ref_noisy(w, chain, normals)


FIR5 = T.fir([0.1, 0.2, 0.4, 0.2, 0.1])
CHAINS = {
    "absolute": [T.noise(25.5)],
    "snr": [T.at(20)],
    "first": [T.noise(40), T.median(3), FIR5, T.quant(4)],
    "middle": [T.median(3), T.at(15), FIR5, T.quant(4)],
    "last": [T.median(3), FIR5, T.quant(4), T.noise(3.25)],
    "two": [T.noise(30), T.median(3), T.noise(30), FIR5],
}


@pytest.mark.parametrize("r", [1, 3])
@pytest.mark.parametrize("name", sorted(CHAINS))
def test_kernel_equals_the_restatement(eng, name, r):
    chain = CHAINS[name]
    wavs = [_rand(n, 10 + i) for i, n in enumerate(LENGTHS)]        # one batch of unequal lengths
    eng.set_input_transform(chain)
    try:
        got = eng.debug_input_transform_eot(wavs, r, SEED, STREAM, EPOCH)
        for b, w in enumerate(wavs):
            for j in range(r):
                want = _want(eng, w, chain, b, j)                    # E_u is checked through the SNR chains' results
                assert got[b][j].dtype == np.int16 and got[b][j].shape == want.shape
                assert np.array_equal(got[b][j], want), (name, w.size, j, int(np.flatnonzero(got[b][j] != want)[0]))
        if r == 3:
            big = got[-1]
            assert not any(np.array_equal(big[a], big[c]) for a, c in ((0, 1), (0, 2), (1, 2)))
        if name == "two":                                           # the two stages draw different normals
            z0 = eng.debug_tf_noise(SEED, STREAM, EPOCH, 5, 0, 0, 0, 4096)
            z2 = eng.debug_tf_noise(SEED, STREAM, EPOCH, 5, 0, 2, 0, 4096)
            assert not np.any(z0 == z2)
        assert any(not np.array_equal(got[b][0], wavs[b]) for b in range(len(wavs)))
    finally:
        eng.set_input_transform(None)


def test_a_silent_utterance_in_snr_mode_stays_silent(eng):
    wavs = [np.zeros(TILE + 9, np.int16), _rand(700, 1)]
    eng.set_input_transform("at:10")
    try:
        got = eng.debug_input_transform_eot(wavs, 2, SEED, STREAM, EPOCH)
    finally:
        eng.set_input_transform(None)
    assert np.array_equal(got[0][0], wavs[0]) and np.array_equal(got[0][1], wavs[0])
    assert not np.array_equal(got[1][0], wavs[1])


def test_full_scale_input_clips(eng):
    w = np.where(np.arange(2 * TILE + 3) % 2 == 0, 32767, -32768).astype(np.int16)
    chain = [T.noise(32768)]
    eng.set_input_transform(chain)
    try:
        got = eng.debug_input_transform_eot([w], 1, SEED, STREAM, EPOCH)[0][0]
    finally:
        eng.set_input_transform(None)
    assert np.array_equal(got, _want(eng, w, chain, 0, 0))
    assert (got == 32767).sum() > w.size // 4 and (got == -32768).sum() > w.size // 4   # both clips fire
    assert ((got > -32768) & (got < 32767)).any()


def test_replication_without_a_chain_is_a_copy(eng):
    eng.set_input_transform(None)
    wavs = [_rand(n, i) for i, n in enumerate((3, TILE + 5, 9000))]
    got = eng.debug_input_transform_eot(wavs, 4, SEED, STREAM, EPOCH)
    for w, reps in zip(wavs, got):
        assert len(reps) == 4 and all(np.array_equal(w, g) for g in reps)


def test_deterministic_chain_through_the_replicating_kernel(eng):
    from tests.input_transform_ref import ref
    chain = T.parse("ms:3,as:5,qt:4")
    wavs = [_rand(n, 20 + i) for i, n in enumerate(LENGTHS)]
    eng.set_input_transform(chain)
    try:
        got = eng.debug_input_transform_eot(wavs, 2, SEED, STREAM, EPOCH)
        plain = eng.debug_input_transform(wavs)
    finally:
        eng.set_input_transform(None)
    for w, reps, p in zip(wavs, got, plain):
        want = ref(w, chain)
        assert np.array_equal(p, want) and np.array_equal(reps[0], want) and np.array_equal(reps[1], want)


# ------------------------------------------------------------------------------------------------- the normals
def test_normals_moments(eng):
    n = 1 << 18
    z = eng.debug_tf_noise(SEED, STREAM, EPOCH, 0, 0, 0, 0, n).astype(np.float64)
    assert np.all(np.isfinite(z))
    assert abs(z.mean()) <= 5.0 / np.sqrt(n)                   # sd of the mean: 1 / sqrt(n)
    assert abs(z.var() - 1.0) <= 5.0 * np.sqrt(2.0 / n)        # sd of the variance of normals: sqrt(2 / n)


def test_a_window_into_the_stream_is_the_same_stream(eng):
    z = eng.debug_tf_noise(SEED, STREAM, EPOCH, 2, 1, 3, 0, 5000)
    for i0, n in ((0, 1), (1, 6), (3, 4), (4, 4), (4093, 10), (4999, 1)):
        w = eng.debug_tf_noise(SEED, STREAM, EPOCH, 2, 1, 3, i0, n)
        assert np.array_equal(w.view(np.uint32), z[i0:i0 + n].view(np.uint32)), (i0, n)


def test_every_word_of_the_key_and_counter_matters(eng):
    n = 2048
    base = dict(seed=SEED, stream=STREAM, epoch=EPOCH, utt=1, replica=0, stage=0)
    z = eng.debug_tf_noise(i0=0, n=n, **base)
    others = {"seed": SEED ^ 1, "seed hi": SEED ^ (1 << 40), "stream": STREAM + 1, "epoch": EPOCH + 1, "utt": 2, "replica": 1,
              "stage": 1}
    for name, v in others.items():
        kw = dict(base)
        kw["seed" if name == "seed hi" else name] = v
        z2 = eng.debug_tf_noise(i0=0, n=n, **kw)
        q, q2 = z.reshape(-1, 4), z2.reshape(-1, 4)              # a row = the four words of one Philox call
        assert not np.any(np.all(q == q2, axis=1)), name
    assert np.array_equal(z, eng.debug_tf_noise(i0=0, n=n, **base))


def test_no_row_shared_with_the_other_streams(eng):
    n = 2048
    seed = 99
    z = eng.debug_tf_noise(seed, 0, 0, 0, 0, 0, 0, n).reshape(-1, 4)
    nes = eng.debug_noise(seed, 0, 0, n, 1).reshape(-1, 4)
    dith = eng.debug_dither_noise(seed, 0, 0, 0, 0, 1, L=n).reshape(-1, 4)
    assert not np.any(np.all(z == nes, axis=1)) and not np.any(np.all(z == dith, axis=1))


# ----------------------------------------------------------------------------------------------------- scoring
def _wav(utt, n=16000):
    return (synthetic_audio(utt, n) * 32768.0).astype(np.int16)


def _check_scoring(d, c, chain):
    wavs = [_wav(0), _wav(1, 12000), _wav(2, 9001)]
    d.set_input_transform(chain)
    d.set_dither_seed(77)
    raw0, tv0 = d.score_raw(wavs)                                   # serial 0
    raw1, _ = d.score_raw(wavs)                                     # serial 1
    for serial, raw in ((0, raw0), (1, raw1)):
        ref_w = [_want(d, w, chain, b, 0, seed=77, stream=0xFFFFFFFF, epoch=serial) for b, w in enumerate(wavs)]
        raw_c, tv_c = c.score_raw(ref_w)
        assert np.array_equal(raw, raw_c), serial
    assert np.array_equal(tv0, tv_c)
    assert not np.array_equal(raw0, raw1)                           # the serial advances: a fresh draw per query
    d.set_dither_seed(77)
    assert np.array_equal(d.score_raw(wavs)[0], raw0)               # the same seed reproduces them
    assert np.array_equal(d.score_raw(wavs)[0], raw1)


@pytest.mark.parametrize("mfcc_f32", [0, 1], ids=["float64 MFCC", "float32 MFCC"])
def test_scoring_through_a_noise_chain_gmm(small_system, mfcc_f32):
    ubm, spk = small_system
    d, c = Engine(0), Engine(0)
    try:
        for e in (d, c):
            e.set_frontend(mfcc_f32=mfcc_f32)
            e.load_gmm([ubm] + spk)
            e.set_system("OSI")
        _check_scoring(d, c, [T.median(3), T.at(20)])
    finally:
        d.close()
        c.close()


def test_scoring_through_a_noise_chain_ivector():
    sy = synthetic_ivector_system(C=96, D=72, R=48, L=24, n_speakers=3, seed=11)
    d, c = Engine(0), Engine(0)
    try:
        d.load_ivector(sy, "OSI")
        c.load_ivector(sy, "OSI")
        _check_scoring(d, c, [T.at(20)])
    finally:
        d.close()
        c.close()


# ---------------------------------------------------------------------------------------------------- refusals
def test_refusals_keep_the_previous_chain(eng):
    kept = [T.noise(5.0), T.quant(8)]
    w = _rand(5000, 4)
    eng.set_input_transform(kept)
    try:
        want = eng.debug_input_transform_eot([w], 1, SEED, STREAM, EPOCH)[0][0]
        bad = {
            "mode 2": T.Stage(T.NOISE, 2, np.array([1.0])), "mode -1": T.Stage(T.NOISE, -1, np.array([1.0])),
            "s < 0": T.Stage(T.NOISE, 0, np.array([-1.0])), "s > 32768": T.Stage(T.NOISE, 0, np.array([32768.5])),
            "s nan": T.Stage(T.NOISE, 0, np.array([np.nan])), "s inf": T.Stage(T.NOISE, 0, np.array([np.inf])),
            "rho 0": T.Stage(T.NOISE, 1, np.array([0.0])), "rho < 0": T.Stage(T.NOISE, 1, np.array([-2.0])),
            "rho nan": T.Stage(T.NOISE, 1, np.array([np.nan])), "rho inf": T.Stage(T.NOISE, 1, np.array([np.inf])),
            "null": T.Stage(T.NOISE, 0, None),
        }
        for name, st in sorted(bad.items()):
            with pytest.raises(NativeError) as ex:
                eng.set_input_transform([T.quant(2), st], validate=False)
            assert ex.value.code == FB_E_ARG, name
            assert np.array_equal(eng.debug_input_transform_eot([w], 1, SEED, STREAM, EPOCH)[0][0], want), name
        eng.set_input_transform([T.Stage(T.NOISE, 0, np.array([32768.0])), T.Stage(T.NOISE, 0, np.array([0.0]))], validate=False)
    finally:
        eng.set_input_transform(None)
