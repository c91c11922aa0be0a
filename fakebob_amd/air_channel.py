"""The over-the-air channel: a random room in front of the victim (fb_set_air_channel; the contract is in
include/fakebob_hip.h).  The engine draws a fresh room impulse response -- direct path, predelay, Gaussian noise under an
exponential decay -- for every (query, row, utterance, draw) and convolves it with the utterance before the input-transform
chain sees it.  The library knows taps, predelay, amp and a range of per-sample decays; this module turns what a person
would say about a room into those numbers:

    spec        "t60:200-600,drr:6,taps:2048,delay:32"        ("none" clears the channel)
    t60         reverberation time in ms, one value or LO-HI: the time in which the tail falls by 60 dB.  Required.
    drr         direct-to-reverberant energy ratio in dB (default 6)
    taps        length L of the response in samples, 2 .. 4096 (default 2048: 128 ms at 16 kHz)
    delay       predelay d in samples, 1 .. L - 1 (default 32): the silence between the direct path and the tail

    rho = 10^(-3 / (t60_ms * fs / 1000))          the per-sample AMPLITUDE decay (60 dB = 3 decades over t60 samples)
    amp = min(16384, 16384 * sqrt((1 - rho_m^2) * 10^(-drr / 10)))     rho_m the mean of the two decays: the tail's
          energy amp^2 / (1 - rho_m^2) stands drr dB under the direct path's 16384^2

The limits are refused here (ValueError) before the call."""
import math

TAPS_MIN, TAPS_MAX = 2, 4096
AMP_MAX = 16384.0
DEFAULT_DRR_DB, DEFAULT_TAPS, DEFAULT_DELAY = 6.0, 2048, 32


class AirChannel(object):
    """fb_air_params as Python holds them: taps, predelay, amp, rho_lo, rho_hi (checked against the contract's limits)."""
    __slots__ = ("taps", "predelay", "amp", "rho_lo", "rho_hi")

    def __init__(self, taps, predelay, amp, rho_lo, rho_hi):
        if not all(isinstance(v, int) or (isinstance(v, float) and math.isfinite(v)) for v in (taps, predelay)) or \
                int(taps) != taps or int(predelay) != predelay:
            raise ValueError("taps and predelay are whole numbers (got %r, %r)" % (taps, predelay))
        self.taps, self.predelay = int(taps), int(predelay)
        self.amp, self.rho_lo, self.rho_hi = float(amp), float(rho_lo), float(rho_hi)
        if not TAPS_MIN <= self.taps <= TAPS_MAX:
            raise ValueError("a room response of %d taps: %d .. %d" % (self.taps, TAPS_MIN, TAPS_MAX))
        if not 1 <= self.predelay <= self.taps - 1:
            raise ValueError("predelay %d outside 1 .. taps - 1 = %d" % (self.predelay, self.taps - 1))
        if not (0.0 <= self.amp <= AMP_MAX):                      # (NaN fails too)
            raise ValueError("amp %r outside 0 .. %g" % (self.amp, AMP_MAX))
        if not (0.0 < self.rho_lo <= self.rho_hi <= 1.0):
            raise ValueError("decay range %r .. %r: 0 < rho_lo <= rho_hi <= 1" % (self.rho_lo, self.rho_hi))

    def __eq__(self, other):
        return isinstance(other, AirChannel) and all(getattr(self, k) == getattr(other, k) for k in self.__slots__)

    def __ne__(self, other):
        return not self == other

    def __repr__(self):
        return "AirChannel(taps=%d, predelay=%d, amp=%r, rho_lo=%r, rho_hi=%r)" % (self.taps, self.predelay, self.amp,
                                                                                  self.rho_lo, self.rho_hi)


def rho_from_t60(t60_ms, fs=16000):
    """The per-sample amplitude decay of a tail that falls by 60 dB in t60_ms milliseconds."""
    t60_ms = float(t60_ms)
    if not (t60_ms > 0.0 and math.isfinite(t60_ms)):
        raise ValueError("t60 of %r ms: a positive, finite time" % (t60_ms,))
    return 10.0 ** (-3.0 / (t60_ms * fs / 1000.0))


def amp_from_drr(drr_db, rho_lo, rho_hi):
    """The tail's amplitude (Q14, per unit normal) that puts its energy drr_db under the direct path's."""
    drr_db = float(drr_db)
    if not math.isfinite(drr_db):
        raise ValueError("drr of %r dB is not finite" % (drr_db,))
    rho_m = 0.5 * (rho_lo + rho_hi)
    return min(AMP_MAX, AMP_MAX * math.sqrt((1.0 - rho_m * rho_m) * 10.0 ** (-drr_db / 10.0)))


def from_room(t60_ms, drr_db=DEFAULT_DRR_DB, taps=DEFAULT_TAPS, delay=DEFAULT_DELAY, fs=16000):
    """An AirChannel for rooms of reverberation time t60_ms -- a number or a (lo, hi) pair, in ms -- at drr_db."""
    lo, hi = (t60_ms, t60_ms) if not isinstance(t60_ms, (tuple, list)) else t60_ms
    if float(lo) > float(hi):
        raise ValueError("t60 range %r-%r: the lower end comes first" % (lo, hi))
    rho_lo, rho_hi = rho_from_t60(lo, fs), rho_from_t60(hi, fs)
    return AirChannel(taps, delay, amp_from_drr(drr_db, rho_lo, rho_hi), rho_lo, rho_hi)


def parse(spec, fs=16000):
    """A spec string, an AirChannel or None -> an AirChannel, or None for no channel ("none", "", None).  ValueError for
    anything the grammar or the contract's limits refuse."""
    if spec is None or isinstance(spec, AirChannel):
        return spec
    if not isinstance(spec, str):
        raise ValueError("an air channel is a spec string, an AirChannel or None, not %r" % (spec,))
    txt = spec.strip().lower()
    if txt in ("", "none", "off"):
        return None
    vals = {}
    for item in txt.split(","):
        key, sep, val = item.strip().partition(":")
        if not sep or key not in ("t60", "drr", "taps", "delay") or key in vals:
            raise ValueError("air channel spec %r: items are t60:MS[-MS], drr:DB, taps:L, delay:D, each once" % (spec,))
        vals[key] = val.strip()
    if "t60" not in vals:
        raise ValueError("air channel spec %r names no t60" % (spec,))
    try:
        lo, sep, hi = vals["t60"].partition("-")
        t60 = (float(lo), float(hi) if sep else float(lo))
        drr = float(vals.get("drr", DEFAULT_DRR_DB))
        taps = int(vals.get("taps", DEFAULT_TAPS))
        delay = int(vals.get("delay", DEFAULT_DELAY))
    except ValueError:
        raise ValueError("air channel spec %r: a number does not parse" % (spec,))
    return from_room(t60, drr, taps, delay, fs)
