"""Companion utterances: one perturbation for several utterances of a speaker (fb_set_companions; the "Composition"
paragraph of include/fakebob_hip.h).  The host side of the contract: the int16 cast, the clip-add that carries a
perturbation over to another recording, the argument handling of Engine.set_companions / FakeBob.attack(companions=...)
and the driver's crop rule.  Nothing here runs on the hot path: the composition inside an attack is the library's."""
import numpy as np

MAX_COMPANIONS = 31     # fb_set_companions: 1 <= K1 <= 31
MAX_REPLICAS = 32       # ... and K * eot <= 32


def cast_i16(audio, bits_per_sample=16):
    """The int16 cast of the NES batch (gmm_ubm_OSI.py:83-85; fb_quantize): (x * 2^(bits - 1)).astype(int16) -- truncation
    toward zero, the low 16 bits kept (1.0 -> -32768).  int16 input is taken as it is."""
    a = np.asarray(audio)
    if a.dtype == np.int16:
        return np.ascontiguousarray(a.reshape(-1))
    v = np.trunc(a.reshape(-1).astype(np.float64) * float(2 ** (int(bits_per_sample) - 1)))
    v = np.where(np.abs(v) < 9.2e18, v, 0.0)    # (NaN and out-of-range values cast to 0, as on the device)
    return (v.astype(np.int64) & 0xFFFF).astype(np.uint16).view(np.int16)


def as_companions(wavs, n=None, bits_per_sample=16):
    """Companions as the library takes them: None / an empty list -> None; else a contiguous int16 array (K1, N) from a list
    (or 2-D array, one row per utterance) of float or int16 utterances of EQUAL length -- n, when given, the length of the
    utterance they ride along with.  ValueError for unequal lengths (nothing is cropped silently: the caller decides what
    to cut), for more than 31 and for empty utterances."""
    if wavs is None:
        return None
    if isinstance(wavs, np.ndarray) and wavs.ndim == 1:
        wavs = [wavs]
    lst = [cast_i16(w, bits_per_sample) for w in wavs]
    if not lst:
        return None
    if len(lst) > MAX_COMPANIONS:
        raise ValueError("%d companions: at most %d" % (len(lst), MAX_COMPANIONS))
    sizes = [a.size for a in lst]
    want = sizes[0] if n is None else int(n)
    if any(s != want for s in sizes):
        raise ValueError("companions must be as long as the attacked utterance (%d samples), got lengths %s: crop them "
                         "yourself (fakebob_amd.companions.crop_to_shortest), nothing is cropped silently" % (want, sizes))
    if want < 1:
        raise ValueError("empty companion utterances")
    return np.ascontiguousarray(np.stack(lst))


def compose(q, a0, wav):
    """The contract's composition on the host: clip(wav + q - a0, -32768, 32767) in int32 arithmetic -> int16."""
    d = np.asarray(q, np.int16).astype(np.int32) - np.asarray(a0, np.int16).astype(np.int32)
    return np.clip(np.asarray(wav, np.int16).astype(np.int32) + d, -32768, 32767).astype(np.int16)


def apply_perturbation(perturbation, wavs, bits_per_sample=16):
    """The perturbation of an attack (adv_i16 - a_0, int32) added to other recordings by the contract's clip-add: a list of
    int16 arrays, one per utterance of wavs (float or int16, each as long as the perturbation)."""
    d = np.asarray(perturbation).reshape(-1).astype(np.int32)
    if isinstance(wavs, np.ndarray) and wavs.ndim == 1:
        wavs = [wavs]
    out = []
    for w in wavs:
        a = cast_i16(w, bits_per_sample)
        if a.size != d.size:
            raise ValueError("utterance of %d samples, perturbation of %d" % (a.size, d.size))
        out.append(np.clip(a.astype(np.int32) + d, -32768, 32767).astype(np.int16))
    return out


def crop_to_shortest(wavs):
    """The driver's crop rule: every utterance cut to the FIRST n samples, n the length of the shortest -> (list, n)."""
    lst = [np.asarray(w).reshape(-1) for w in wavs]
    n = min(a.size for a in lst)
    return [a[:n] for a in lst], n


def pick_companions(items, idx, count):
    """The driver's choice: the next `count` DISTINCT utterances of the same speaker after items[idx] in the data
    directory's (sorted) order, wrapping around; fewer when the speaker has fewer.  -> indices into items."""
    me = items[idx]
    same = [i for i, it in enumerate(items) if it["spk"] == me["spk"]]
    seen, out = {me["name"]}, []
    at = same.index(idx)
    for k in range(1, len(same)):
        i = same[(at + k) % len(same)]
        if items[i]["name"] in seen:
            continue        # (a targeted job lists a file once per target)
        seen.add(items[i]["name"])
        out.append(i)
        if len(out) == count:
            break
    return out


def succeeded(task, attack_type, decision, target=None, true=None):
    """Whether a decision of model.make_decisions is what the attack wanted."""
    d = int(decision)
    if task == "SV":
        return d == 1
    if attack_type == "targeted":
        return d == int(target)
    return d != int(true) if task == "CSI" else d != -1


class AttackResult(tuple):
    """What FakeBob.attack returns: the reference's pair (int16 adversarial audio (N, 1), success flag) -- it unpacks as
    before -- with the universal-perturbation view of the same attack:
      perturbation_i16  adv_i16 - a_0, a_0 the int16 cast of the attacked audio (int32 storage: a difference of two int16)
      apply_perturbation(wavs)  the contract's clip-add of it onto other recordings -> a list of int16 arrays
      per_utterance     with companions: one dict per composed utterance (0 = the attacked one) -- audio_i16, score and
                        decision from the system's ordinary score / make_decisions, success; None without companions
      per_offset        after an attack under a play offset (FakeBob(play_offset=S)) only -- the attribute is absent otherwise:
                        one dict per utterance with the perturbation re-scored at each offset of play_offset.offset_grid(S)
      apply_perturbation(wavs, offset=t)  the perturbation rotated circularly by t samples first (play_offset.compose)
    The flag is the loop's: it reads the MEAN loss over the utterances; per_utterance says which of them succeeded."""

    def __new__(cls, adv, flag, perturbation, bits_per_sample=16, per_utterance=None, per_offset=None):
        self = tuple.__new__(cls, (adv, flag))
        self.perturbation_i16 = perturbation
        self.bits_per_sample = bits_per_sample
        self.per_utterance = per_utterance
        if per_offset is not None:
            self.per_offset = per_offset
        return self

    def apply_perturbation(self, wavs, offset=0):
        if offset == 0:
            return apply_perturbation(self.perturbation_i16, wavs, self.bits_per_sample)
        from .play_offset import apply_perturbation as rotated
        return rotated(self.perturbation_i16, wavs, offset, self.bits_per_sample)
