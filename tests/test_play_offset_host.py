"""The play offset on the host (fb_set_play_offset; the "Play offset" section of include/fakebob_hip.h): the numpy restatement
(tests/play_offset_ref.py) against the product's host module (fakebob_amd/play_offset.py) bit for bit, the range of the draw,
S = 0 as the companions composition, the adjoint identity of the transposed rule, the driver's refusals and --play-offset max,
and -- on the restatement alone -- that the fixed cases of tests/test_gpu_play_offset.py cannot pass vacuously."""
import contextlib
import io
import os

import numpy as np
import pytest

from fakebob_amd import attack_main as AM, play_offset as PO
from tests import companions_ref as CR, play_offset_ref as R
from tests.golden import driver_site as DS
from tests.play_offset_cases import BIT_CASES, POINT, ROWS

SEED, STREAM, EPOCH = POINT


@pytest.fixture(scope="module")
def philox(oracle):
    return oracle.philox


def _rows(n, K1, seed=0):
    """a0, one perturbed NES row and K1 companions with samples at the rails, so that the clip acts on either side"""
    rng = np.random.default_rng(1000 + n + seed)
    a0 = rng.integers(-3000, 3001, n).astype(np.int16)
    comp = rng.integers(-3000, 3001, (K1, n)).astype(np.int16)
    q = np.clip(a0.astype(np.int32) + rng.integers(-70, 71, n), -32768, 32767).astype(np.int16)
    for p in {0, n // 2, n - 1}:
        a0[p] = 32767 if p % 2 == 0 else -32768
        if K1:
            comp[0, p], comp[-1, p] = 32767, -32768
    return q, a0, comp


def test_the_products_philox_is_the_oracles(philox):
    rng = np.random.default_rng(5)
    for _ in range(64):
        ctr = [int(x) for x in rng.integers(0, 2 ** 32, 4)]
        key = [int(x) for x in rng.integers(0, 2 ** 32, 2)]
        assert PO.philox4x32_10(ctr, key) == [int(w) for w in philox(ctr, key)]
    assert PO.philox4x32_10([0, 0, 0, 0], [0, 0]) == [int(w) for w in philox([0, 0, 0, 0], [0, 0])]


@pytest.mark.parametrize("S", [1, 7, 3999, 2 ** 31 - 2])
def test_the_draw_agrees_and_stays_in_range(philox, S):
    seen = set()
    for seed in (SEED, 2 ** 40 + 17):
        for b in range(12):
            for rho in range(32):
                t = R.draw(philox, seed, STREAM, EPOCH, b, rho, S)
                assert t == PO.draw(seed, STREAM, EPOCH, b, rho, S)
                assert 0 <= t <= S
                seen.add(t)
    assert 0 in seen or S > 7
    if S <= 7:
        assert seen == set(range(S + 1))                       # both ends are reached
    else:
        assert min(seen) < S // 8 and max(seen) > S - S // 8   # ... and the whole range is used
    assert R.draw(philox, SEED, STREAM + 1, EPOCH, 0, 0, 2 ** 31 - 2) != R.draw(philox, SEED, STREAM, EPOCH, 0, 0, 2 ** 31 - 2)
    for bad in (-1, 2 ** 31 - 1):
        with pytest.raises(ValueError):
            PO.draw(SEED, STREAM, EPOCH, 0, 0, bad)


def test_offset_zero_is_the_companions_composition():
    q, a0, comp = _rows(257, 2)
    want = CR.compose_row(q, a0, comp)                          # utterance 0: q itself
    got = R.compose_rows(q, a0, comp, 1, [0, 0, 0])
    assert np.array_equal(got, want)
    assert np.array_equal(R.compose_rows(a0, a0, comp, 2, [5, 200, 1, 256, 0, 77]), np.repeat(np.concatenate([a0[None], comp]), 2, axis=0))


@pytest.mark.parametrize("n", [1, 2, 257, 4001])
def test_the_products_compose_is_the_restatements(n):
    q, a0, comp = _rows(n, 1)
    delta = q.astype(np.int32) - a0.astype(np.int32)
    for tau in sorted({0, 1 % n, n // 3, n - 1}):
        for host in (a0, comp[0]):
            assert np.array_equal(PO.compose(host, delta, tau), R.compose_one(host, q, a0, tau))
    with pytest.raises(ValueError):
        PO.compose(a0, delta, n)
    with pytest.raises(ValueError):
        PO.compose(a0.astype(np.int32), delta, 0)
    assert PO.offset_grid(4000) == [(k * 4000) // 15 for k in range(16)] and PO.offset_grid(4000)[0] == 0 and PO.offset_grid(4000)[-1] == 4000
    assert PO.offset_grid(5) == [0, 1, 2, 3, 4, 5] and PO.offset_grid(200, 3) == [0, 100, 200]


@pytest.mark.parametrize("n,K1,eot", [(1, 0, 1), (2, 1, 1), (257, 2, 2), (4001, 1, 3)])
def test_the_adjoint_identity_is_exact_on_integers(n, K1, eot):
    """<compose'(delta), c> == <delta, compose_t(c)> with integer cotangents small enough for float64 to add exactly, clipped
    samples (m = 0) included -- at the wrap too"""
    rng = np.random.default_rng(n)
    q, a0, comp = _rows(n, K1)
    R_ = (K1 + 1) * eot
    tau = rng.integers(0, n, R_)
    tau[0], tau[-1] = 0, n - 1
    if K1:                                                      # a clipped sample exactly where replica R_ - 1 wraps
        i = int(tau[-1]) % n
        comp[-1, i], q[(i - int(tau[-1])) % n], a0[(i - int(tau[-1])) % n] = 32767, 100, 0
    m = R.mask(q, a0, comp, eot, tau)
    assert K1 == 0 or not m.all()
    cot = rng.integers(-1000, 1001, (R_, n)).astype(np.float64)
    delta = rng.integers(-50, 51, n)
    lhs = int((R.compose_linear(delta, q, a0, comp, eot, tau) * cot.astype(np.int64)).sum())
    g = R.compose_t(cot, q, a0, comp, eot, tau)
    assert np.array_equal(g, np.rint(g))
    assert lhs == int((delta * g.astype(np.int64)).sum())
    # the derivative is the composition's: a step of +-1 where nothing clips moves the composed rows by exactly that
    rows = R.compose_rows(q, a0, comp, eot, tau).astype(np.int64)
    step = np.where((q < 32767) & (q > -32768), 1, 0).astype(np.int16)
    moved = R.compose_rows((q + step).astype(np.int16), a0, comp, eot, tau).astype(np.int64)
    lin = R.compose_linear(step, q, a0, comp, eot, tau)
    inside = R.mask((q + step).astype(np.int16), a0, comp, eot, tau) & m
    assert np.array_equal((moved - rows)[inside], lin[inside])


def test_the_fixed_gpu_cases_are_not_vacuous(philox):
    """Every case of tests/test_gpu_play_offset.py with more than one replica per NES row draws at least two distinct offsets
    for every NES row, and every case with S = n - 1 has at least one offset whose wrap falls strictly inside a workgroup's
    tile; the cases together cover a wrap in the row's first chunk (S = 1) and offsets 0 .. 7 inside one 16-byte store."""
    first_chunk = False
    for stage, n, S, K, eot in BIT_CASES:
        r = K * eot
        tau = R.offsets(philox, SEED, STREAM, EPOCH, ROWS, r, S)
        assert tau.min() >= 0 and tau.max() <= S
        if r > 1:
            assert all(len(set(row)) >= 2 for row in tau.tolist()), (stage, n, S, K, eot, tau)
        if S == n - 1:
            inside = [R.wraps_inside_a_tile(n, b * r + rho, int(tau[b, rho])) for b in range(ROWS) for rho in range(r)]
            assert any(inside), (stage, n, S, K, eot)
            if r > 1:
                assert (tau % 2 == 1).any() and (tau % 2 == 0).any()      # both alignments of the rotated source
        first_chunk |= S == 1 and bool((tau == 1).any())
    assert first_chunk


def test_the_composing_kernel_uses_no_scratch(tmp_path):
    """k_play_compose is a stream: the compiler's own figures (the flags of fakebob_amd.build, device-only,
    -Rpass-analysis=kernel-resource-usage, as tests/test_kernel_footprints.py reads them) show no scratch and no spilled register
    for it and for its transpose"""
    import re
    import subprocess
    from fakebob_amd import build as B
    src = "play_offset_kernels.hip"
    assert src in B.SOURCES
    cmd = ([B._hipcc()] + B.FLAGS + B.SOURCE_FLAGS.get(src, []) +
           ["--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(B.CSRC, src), "-o", str(tmp_path / "po.o")])
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-4000:]
    usage, cur = {}, None
    for m in re.finditer(r"remark:\s+([A-Za-z][^:\n]*): (\S+) \[-Rpass-analysis=kernel-resource-usage\]", r.stdout):
        key, val = m.group(1).strip(), m.group(2)
        if key == "Function Name":
            cur = usage.setdefault(val, {})
        elif cur is not None and key in ("ScratchSize [bytes/lane]", "VGPRs Spill", "SGPRs Spill"):
            cur[key] = int(val)
    for prefix in ("_Z14k_play_compose", "_Z19k_wb_play_compose_t"):
        (name,) = [k for k in usage if k.startswith(prefix)]
        assert usage[name] == {"ScratchSize [bytes/lane]": 0, "VGPRs Spill": 0, "SGPRs Spill": 0}, (name, usage[name])


# ------------------------------------------------------------------------------------------------ the driver
class _Engine(object):
    def stats(self):
        return dict(nes_iters=0, scored_utts=0)

    def set_fused_chain(self, on):
        pass


class _Native(DS.StubModel):
    """a stub with an engine: the driver takes it for one of the engine's own systems"""
    def __init__(self, task, threshold=0.0):
        DS.StubModel.__init__(self, task, threshold)
        self.engine = _Engine()


class _Bob(DS.StubBob):
    def attack(self, audio, checkpoint_path, **kw):
        kw.pop("companions", None)
        DS.StubBob.log.append(("play", getattr(self, "play_offset", None), np.asarray(audio).reshape(-1).size))
        return DS.StubBob.attack(self, audio, checkpoint_path, **kw)


@pytest.fixture()
def site(tmp_path):
    DS.make_site(str(tmp_path))
    old = os.getcwd()
    os.chdir(str(tmp_path))
    yield str(tmp_path)
    os.chdir(old)


def _main(extra, native=True):
    built = []

    def model(archi, t, ml, pre, th, gid):
        built.append(gid)
        return (_Native if native else DS.StubModel)(t, th)
    DS.StubBob.log = []
    argv = ["-spk_id"] + DS.SPK_IDS + ["-task", "OSI", "-type", "targeted", "--streams", "1", "--seed", "5"] + extra
    err = io.StringIO()
    with contextlib.redirect_stdout(io.StringIO()), contextlib.redirect_stderr(err):
        try:
            res = AM.main(argv, model_factory=model, bob_factory=lambda task, at, m, **hp: _Bob(task, at, m, **hp))
        except SystemExit:
            return None, built, err.getvalue()
    return res, built, err.getvalue()


@pytest.mark.parametrize("attack", ["pso", "kenansville", "hsj", "cw2", "psy"])
def test_the_driver_refuses_the_other_attacks_by_name(site, attack):
    res, built, err = _main(["--attack", attack, "--play-offset", "100"])
    assert res is None and not built and "--play-offset" in err and "--attack %s" % attack in err, err


def test_the_driver_rules(site):
    res, built, err = _main(["--attack", "pgd", "--play-offset", "max"])
    assert res is None and not built and "--wb-universal" in err and "--play-offset" in err, err
    for bad in ("-1", "2147483647", "most"):
        res, built, err = _main(["--play-offset", bad])
        assert res is None and not built and "--play-offset" in err, (bad, err)
    res, built, err = _main(["--play-offset", "max"], native=False)          # a foreign model: refused in Python
    assert res is None and "--play-offset" in err and "foreign" in err, err
    res, _b, err = _main(["--play-offset", "max"])
    assert res is not None, err
    plays = [e for e in DS.StubBob.log if e[0] == "play"]
    assert plays and all(p[1] == p[2] - 1 == 799 for p in plays)              # max: N - 1 of every utterance
    res, _b, err = _main(["--attack", "pgd", "--wb-universal", "--play-offset", "12"])
    assert res is not None, err
    assert all(e[1] == 12 for e in DS.StubBob.log if e[0] == "play")
    res, _b, err = _main([])                                                   # without the option nothing is set
    assert res is not None and all(e[1] is None for e in DS.StubBob.log if e[0] == "play")
    assert PO.parse_option("max", 4000) == 3999 and PO.parse_option("17", 4000) == 17 and PO.parse_option(None, 4000) == 0
    with pytest.raises(ValueError):
        PO.parse_option("4000", 4000)


def test_the_python_classes_refuse_what_the_library_does_not_model():
    from fakebob_amd.attack import FakeBob
    with pytest.raises(ValueError, match="foreign"):
        FakeBob("OSI", "targeted", DS.StubModel("OSI"), play_offset=10, verbose=False)
    FakeBob("OSI", "targeted", DS.StubModel("OSI"), play_offset=None, verbose=False)
    with pytest.raises(ValueError):
        FakeBob("OSI", "targeted", DS.StubModel("OSI"), play_offset=2 ** 31 - 1, verbose=False)
