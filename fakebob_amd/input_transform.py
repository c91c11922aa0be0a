"""Input-transform chains of a defended system: the stages the engine applies to every utterance its own front end
reads, between the int16 cast and the MFCC (fb_set_input_transform; the stage contract is in include/fakebob_hip.h).

The input transformations FAKEBOB's evaluation places in front of the recogniser -- quantisation, local median
smoothing, down-sampling ("audio squeezing") -- and the filters of the same family (average smoothing, low-pass
filters, a room impulse response) are all chains of four int16 -> int16 stage kinds; the fifth kind, additive white
Gaussian noise (SpeakerGuard's AT), makes the victim randomised: it draws afresh at every query, and the attack answers
with expectation over transformation (Engine.set_eot, eot_size=).  This module builds the stages
(the filter taps with numpy: the engine takes them as data), parses the short spec strings the system classes and the
driver accept, and checks the engine's limits before the call.

    spec     ::= stage ("," stage)*  |  ""  |  "none"
    qt:q     quantisation to multiples of q                       quant(q)
    ms:k     median smoothing over k samples (odd)                median(k)
    as:k     average smoothing over k samples (odd)               average(k)
    lpf:f    windowed-sinc low-pass at f Hz (lpf:f:L for L taps)  lowpass(f, L)
    ds:q     audio squeezing: down-sample by q and back           squeeze(q)   (three stages)
    dec:q    keep every q-th sample, zero the others              decimate(q)
    noise:s  white Gaussian noise of standard deviation s LSBs    noise(s)
    at:snr   white Gaussian noise at snr dB below the utterance   at(snr_db)
"""
import collections

import numpy as np

QUANT, MEDIAN, FIR, DECIMATE, NOISE = 0, 1, 2, 3, 4
NOISE_ABS, NOISE_SNR = 0, 1   # a noise stage's k: taps[0] is the amplitude s / rho = 10^(snr_db / 10)
MAX_STAGES = 8
MAX_HALO = 1024       # largest sum of the stages' radii
MAX_TAP = 2.0 ** 20   # largest tap magnitude

Stage = collections.namedtuple("Stage", "kind k taps")


def radius(stage):
    return (stage.k - 1) // 2 if stage.kind in (MEDIAN, FIR) else 0


def quant(q):
    q = int(q)
    if not 1 <= q <= 16384:
        raise ValueError("quantisation step %d outside 1 .. 16384" % q)
    return Stage(QUANT, q, None)


def median(k):
    k = int(k)
    if not 3 <= k <= 31 or k % 2 == 0:
        raise ValueError("median width %d is not odd in 3 .. 31" % k)
    return Stage(MEDIAN, k, None)


def fir(taps):
    taps = np.ascontiguousarray(taps, np.float64).reshape(-1)
    if not 1 <= taps.size <= 511 or taps.size % 2 == 0:
        raise ValueError("FIR length %d is not odd in 1 .. 511" % taps.size)
    if not np.all(np.isfinite(taps)) or np.max(np.abs(taps)) > MAX_TAP:
        raise ValueError("FIR taps must be finite and at most 2^20 in magnitude")
    return Stage(FIR, int(taps.size), taps)


def decimate(q):
    q = int(q)
    if not 2 <= q <= 64:
        raise ValueError("decimation factor %d outside 2 .. 64" % q)
    return Stage(DECIMATE, q, None)


def _noise_stage(mode, value):
    """A noise stage from its mode and parameter, inside the library's limits (the C refusals, mirrored)."""
    mode = int(mode)
    if mode not in (NOISE_ABS, NOISE_SNR):
        raise ValueError("noise mode %d is neither 0 (absolute) nor 1 (SNR)" % mode)
    v = float(value)
    if mode == NOISE_ABS and not 0.0 <= v <= 32768.0:       # (NaN fails the comparisons too)
        raise ValueError("noise amplitude %g is not in 0 .. 32768" % v)
    if mode == NOISE_SNR and not (v > 0.0 and np.isfinite(v)):
        raise ValueError("rho = %g (10^(snr_db / 10)) is not finite and positive" % v)
    return Stage(NOISE, mode, np.array([v], np.float64))


def noise(s):
    """White Gaussian noise of standard deviation s (int16 LSBs, 0 .. 32768), drawn afresh at every query."""
    return _noise_stage(NOISE_ABS, s)


def at(snr_db):
    """SpeakerGuard's AT: white Gaussian noise snr_db decibels below the utterance's own power, drawn afresh at every query.
    The stage carries rho = 10 ** (snr_db / 10)."""
    snr_db = float(snr_db)
    if not np.isfinite(snr_db):
        raise ValueError("SNR %g dB is not finite" % snr_db)
    return _noise_stage(NOISE_SNR, 10.0 ** (snr_db / 10))


def average(k):
    """Average smoothing over k samples (odd): FIR with taps 1 / k."""
    k = int(k)
    if k % 2 == 0:
        raise ValueError("average width %d is not odd" % k)
    return fir(np.full(k, 1.0 / k))


def lowpass_taps(cutoff_hz, L=101, fs=16000.0, gain=1.0):
    """Hamming-windowed sinc low-pass, L taps (odd), unit gain at 0 Hz times `gain`."""
    L = int(L)
    if L % 2 == 0 or L < 1:
        raise ValueError("low-pass length %d is not odd" % L)
    if not 0.0 < cutoff_hz <= fs / 2:
        raise ValueError("cut-off %g Hz outside (0, fs / 2]" % cutoff_hz)
    t = np.arange(L, dtype=np.float64) - (L - 1) // 2
    h = np.sinc(2.0 * cutoff_hz / fs * t) * (np.hamming(L) if L > 1 else 1.0)
    return h * (gain / h.sum())


def lowpass(cutoff_hz, L=101, fs=16000.0):
    return fir(lowpass_taps(cutoff_hz, L, fs))


def squeeze(q, L=101, fs=16000.0):
    """Audio squeezing by q: anti-alias low-pass at fs / (2 q), keep every q-th sample, interpolate back with the same
    filter at gain q.  Three stages."""
    q = int(q)
    cut = fs / (2.0 * q)
    return [fir(lowpass_taps(cut, L, fs)), decimate(q), fir(lowpass_taps(cut, L, fs, gain=float(q)))]


def _flatten(stages):
    out = []
    for s in stages:
        if isinstance(s, Stage):
            out.append(s)
        else:
            out.extend(_flatten(s))
    return out


def parse(spec):
    """A spec string (module docstring), a Stage, a (nested) list of stages or None -> a validated list of stages."""
    if spec is None:
        return []
    if isinstance(spec, Stage):
        return validate([spec])
    if not isinstance(spec, str):
        return validate(_flatten(spec))
    spec = spec.strip()
    if spec in ("", "none"):
        return []
    out = []
    for item in spec.split(","):
        f = item.strip().split(":")
        name, args = f[0], f[1:]
        try:
            if name == "qt" and len(args) == 1:
                out.append(quant(int(args[0])))
            elif name == "ms" and len(args) == 1:
                out.append(median(int(args[0])))
            elif name == "as" and len(args) == 1:
                out.append(average(int(args[0])))
            elif name == "dec" and len(args) == 1:
                out.append(decimate(int(args[0])))
            elif name == "ds" and len(args) in (1, 2):
                out.extend(squeeze(int(args[0]), *[int(a) for a in args[1:]]))
            elif name == "noise" and len(args) == 1:
                out.append(noise(float(args[0])))
            elif name == "at" and len(args) == 1:
                out.append(at(float(args[0])))
            elif name == "lpf" and len(args) in (1, 2):
                out.append(lowpass(float(args[0]), *[int(a) for a in args[1:]]))
            else:
                raise ValueError("unknown stage")
        except ValueError as ex:
            raise ValueError("input transform %r: %s" % (item.strip(), ex))
    return validate(out)


def validate(stages):
    """The engine's limits, checked before the call: at most 8 stages, radii summing to at most 1024, every stage inside
    its own range (the builders check that; a hand-made Stage is rebuilt through them)."""
    build = {QUANT: lambda s: quant(s.k), MEDIAN: lambda s: median(s.k), DECIMATE: lambda s: decimate(s.k)}
    out = []
    for s in stages:
        if not isinstance(s, Stage):
            raise TypeError("not a stage: %r" % (s,))
        if s.kind == FIR:
            t = fir(s.taps)
            if t.k != int(s.k):
                raise ValueError("FIR stage says %d taps and carries %d" % (s.k, t.k))
            out.append(t)
        elif s.kind == NOISE:
            if s.taps is None or np.size(s.taps) != 1:
                raise ValueError("a noise stage carries one parameter")
            out.append(_noise_stage(s.k, np.ravel(s.taps)[0]))
        elif s.kind in build:
            out.append(build[s.kind](s))
        else:
            raise ValueError("unknown stage kind %r" % (s.kind,))
    if len(out) > MAX_STAGES:
        raise ValueError("%d stages: an input-transform chain has at most %d" % (len(out), MAX_STAGES))
    halo = sum(radius(s) for s in out)
    if halo > MAX_HALO:
        raise ValueError("the stages' radii sum to %d: at most %d" % (halo, MAX_HALO))
    return out


def c_stages(stages):
    """(ctypes array of fb_tf_stage, objects to keep alive during the call) for a list of stages, unchecked."""
    import ctypes as C
    from . import _native as N
    arr = (N.TfStage * max(1, len(stages)))()
    keep = []
    for i, s in enumerate(stages):
        arr[i].kind, arr[i].k = int(s.kind), int(s.k)
        if s.taps is not None:
            t = np.ascontiguousarray(s.taps, np.float64)
            keep.append(t)
            arr[i].taps = t.ctypes.data_as(C.POINTER(C.c_double))
    return arr, keep
