"""Engine: one GPU + one HIP stream worth of device state behind the C ABI.

Thin numpy <-> pointer marshalling only; all arithmetic of the hot path runs
in libfakebob_hip.so.
"""
import ctypes as C

import numpy as np

from . import _native as N
from .models import stack_models


def nes_params(task, attack_type, adver_thresh=0., epsilon=0.002, max_iter=1000, max_lr=0.001,
               min_lr=1e-6, samples_per_draw=50, sigma=0.001, momentum=0.9, plateau_length=5,
               plateau_drop=2., threshold=0., target=None, true=None, seed=42, stream=0, bits_per_sample=16):
    p = N.NesParams()
    p.task = N.TASK[task]
    p.attack_type = N.ATTACK[attack_type]
    p.adver_thresh = float(adver_thresh); p.epsilon = float(epsilon); p.max_iter = int(max_iter)
    p.max_lr = float(max_lr); p.min_lr = float(min_lr); p.samples_per_draw = int(samples_per_draw)
    p.sigma = float(sigma); p.momentum = float(momentum); p.plateau_length = int(plateau_length)
    p.plateau_drop = float(plateau_drop); p.threshold = float(threshold)
    p.target = 0 if target is None else int(target)
    p.true_label = 0 if true is None else int(true)
    p.seed = int(seed); p.stream = int(stream)
    p.bits_per_sample = int(bits_per_sample)
    return p


def pso_params(particles=25, w_init=0.9, w_end=0.1, c1=1.4961, c2=1.4961, v_max=0.002):
    """fb_pso_params: the swarm of Engine.attack_pso (fakebob_hip.h, "particle-swarm attack")."""
    q = N.PsoParams()
    q.particles = int(particles)
    q.w_init = float(w_init); q.w_end = float(w_end); q.c1 = float(c1); q.c2 = float(c2); q.v_max = float(v_max)
    return q


def cw2_params(initial_const=1e-3, search_steps=9, lr=1e-2, beta1=0.9, beta2=0.999, adam_eps=1e-8, abort_every=1000):
    """fb_cw2_params: the search of Engine.attack_cw2 (fakebob_hip.h, "CW2"); SpeakerGuard's and torch.optim.Adam's defaults."""
    q = N.Cw2Params()
    q.initial_const = float(initial_const); q.search_steps = int(search_steps); q.lr = float(lr)
    q.beta1 = float(beta1); q.beta2 = float(beta2); q.adam_eps = float(adam_eps); q.abort_every = int(abort_every)
    return q


def psy_params(theta, psd_max, window=2048, l2_weight=0.0):
    """fb_psy_params: the masking threshold of Engine.attack_psy (fakebob_hip.h, "masking"; fakebob_amd.masking computes theta
    and psd_max).  The structure keeps theta alive."""
    theta = np.ascontiguousarray(theta, np.float64)
    if theta.ndim != 2:
        raise ValueError("psy_params: theta must be [F, K]")
    m = N.PsyParams()
    m._theta = theta
    m.theta = theta.ctypes.data
    m.n_frames = int(theta.shape[0]); m.window = int(window); m.psd_max = float(psd_max); m.l2_weight = float(l2_weight)
    if theta.shape[1] != m.window // 2 + 1:
        raise ValueError("psy_params: theta has %d bins, window %d has %d" % (theta.shape[1], m.window, m.window // 2 + 1))
    return m


def kv_params(window=100, grid=15, q_max=65536, max_rounds=32):
    """fb_kv_params: the search of Engine.attack_kenansville (fakebob_hip.h, "decision-only attack")."""
    k = N.KvParams()
    k.window = int(window); k.grid = int(grid); k.q_max = int(q_max); k.max_rounds = int(max_rounds)
    return k


def hsj_params(grid=15, max_rounds=8, num_evals_init=32, num_evals_max=256, max_queries=0, sigma_min=2.0 ** -15,
               probe_scale=0.05):
    """fb_hsj_params: the search of Engine.attack_hsj (fakebob_hip.h, "decision-only attack II")."""
    k = N.HsjParams()
    k.grid = int(grid); k.max_rounds = int(max_rounds); k.num_evals_init = int(num_evals_init)
    k.num_evals_max = int(num_evals_max); k.max_queries = int(max_queries)
    k.sigma_min = float(sigma_min); k.probe_scale = float(probe_scale)
    return k


class Engine(object):
    def __init__(self, device=0):
        self._L = N.lib()
        self._h = C.c_void_p()
        N.check(self._L.fb_engine_create(C.c_int(device), C.byref(self._h)))
        self.device = device
        self.task = "OSI"
        self.n_models = 0
        self.cfg = N.FrontendCfg()
        self._L.fb_default_frontend(C.byref(self.cfg))
        self.input_transform = []
        self.air_channel = None
        self.codec = None
        self.eot = 1
        self.wb_bpda = False
        self.wb_ivector = False
        self.wb_xvector = False
        self.wb_air = False
        self.wb_frontend = False
        self.wb_universal = False
        self.companions = None
        self.play_offset = 0
        self.query_eot = None
        self.feature_compression = None

    def close(self):
        if self._h:
            self._L.fb_engine_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- configuration
    def set_frontend(self, **over):
        old = {}
        for k, v in over.items():
            if not hasattr(self.cfg, k):
                raise KeyError(k)
            old[k] = getattr(self.cfg, k)
            setattr(self.cfg, k, v)
        try:
            N.check(self._L.fb_set_frontend(self._h, C.byref(self.cfg)))
        except Exception:
            for k, v in old.items():      # the engine kept its previous configuration: so does the mirror
                setattr(self.cfg, k, v)
            raise

    def set_dither_seed(self, seed):
        """The dither key of scoring calls outside an attack (fb_set_dither_seed); restarts their serial at 0, so the same
        sequence of scoring calls after it draws the same noise."""
        N.check(self._L.fb_set_dither_seed(self._h, C.c_uint64(int(seed))))

    def set_input_transform(self, stages, validate=True):
        """The input-transform chain of a defended system (fb_set_input_transform): a spec string ("ms:7,qt:512"), a list of
        fakebob_amd.input_transform stages, or None / [] / "none" to clear it.  The engine applies it to every utterance its
        own front end reads -- scoring, enrolment statistics, the NES loops --, not to the batch of a foreign model and not
        to the returned audio.  The limits are checked here before the call (ValueError); validate=False hands the stages
        to the library as they are (it refuses what is outside the contract and keeps the previous chain)."""
        from . import input_transform as T
        stages = T.parse(stages) if validate else list(stages or [])
        arr, keep = T.c_stages(stages)
        N.check(self._L.fb_set_input_transform(self._h, arr, C.c_int(len(stages))))
        self.input_transform = stages
        del keep

    def debug_input_transform(self, audio_list):
        """The int16 batch the MFCC would read for these int16 utterances (fb_debug_input_transform): a list of arrays."""
        lst = [np.ascontiguousarray(a, np.int16).reshape(-1) for a in audio_list]
        off = np.zeros(len(lst) + 1, np.int64)
        off[1:] = np.cumsum([a.size for a in lst])
        cat = np.ascontiguousarray(np.concatenate(lst))
        out = np.empty_like(cat)
        N.check(self._L.fb_debug_input_transform(self._h, N.ptr(cat), N.ptr(off), C.c_int(len(lst)), N.ptr(out)))
        return [out[off[i]:off[i + 1]].copy() for i in range(len(lst))]

    def set_air_channel(self, channel, validate=True):
        """The over-the-air channel (fb_set_air_channel): a spec string ("t60:200-600,drr:6,taps:2048,delay:32"), a
        fakebob_amd.air_channel.AirChannel, or None / "none" to clear it.  The engine then convolves every utterance its own
        front end reads -- scoring, enrolment statistics, every NES batch, the PSO swarm -- with a random room impulse response
        drawn afresh per (query, row, utterance, draw), directly in front of the input-transform chain; not the batch of a
        foreign model and not the returned audio.  The limits are checked here before the call (ValueError); validate=False
        hands a (taps, predelay, amp, rho_lo, rho_hi) tuple to the library as it is (it refuses what is outside the contract
        and keeps the previous setting)."""
        from . import air_channel as A
        if validate:
            ch = A.parse(channel)
            vals = None if ch is None else (ch.taps, ch.predelay, ch.amp, ch.rho_lo, ch.rho_hi)
        else:
            ch = vals = channel
        if vals is None:
            N.check(self._L.fb_set_air_channel(self._h, None))
        else:
            p = N.AirParams(int(vals[0]), int(vals[1]), float(vals[2]), float(vals[3]), float(vals[4]))
            N.check(self._L.fb_set_air_channel(self._h, C.byref(p)))
        self.air_channel = ch

    def debug_air_taps(self, seed, stream, epoch, utt=0, replica=0):
        """What k_air_taps writes for one row under the channel set (fb_debug_air_taps): (taps int16 (L,), the float32
        normals z (L,), the decay's 32-bit word w)."""
        if self.air_channel is None:
            raise ValueError("no air channel is set")
        L = int(self.air_channel[0] if isinstance(self.air_channel, tuple) else self.air_channel.taps)
        taps, z, w = np.empty(L, np.int16), np.empty(L, np.float32), C.c_uint32(0)
        N.check(self._L.fb_debug_air_taps(self._h, C.c_uint64(int(seed)), C.c_uint32(int(stream)), C.c_uint32(int(epoch)),
                                          C.c_uint32(int(utt)), C.c_int(int(replica)), N.ptr(taps), N.ptr(z), C.byref(w)))
        return taps, z, int(w.value)

    def debug_air_convolve(self, audio_list, taps):
        """k_air_conv on taps handed in as they are (fb_debug_air_convolve): int16 utterances of any length >= 1 and int16 taps
        (B, L), one response per utterance; a list of int16 arrays."""
        lst = [np.ascontiguousarray(a, np.int16).reshape(-1) for a in audio_list]
        taps = np.ascontiguousarray(taps, np.int16)
        taps = taps.reshape(1, -1) if taps.ndim == 1 else taps
        if taps.shape[0] != len(lst):
            raise ValueError("%d responses for %d utterances" % (taps.shape[0], len(lst)))
        off = np.zeros(len(lst) + 1, np.int64)
        off[1:] = np.cumsum([a.size for a in lst])
        cat = np.ascontiguousarray(np.concatenate(lst))
        out = np.empty_like(cat)
        N.check(self._L.fb_debug_air_convolve(self._h, N.ptr(cat), N.ptr(off), C.c_int(len(lst)), N.ptr(taps),
                                              C.c_int(taps.shape[1]), N.ptr(out)))
        return [out[off[i]:off[i + 1]].copy() for i in range(len(lst))]

    def set_codec(self, codec, validate=True):
        """The telephone-line codec (fb_set_codec): "ulaw", "alaw", "adpcm", or None / "none" to clear it.  The engine then
        sends every row its own front end reads -- scoring, enrolment statistics, every NES batch, the PSO swarm -- through
        the codec's encode / decode round trip, directly behind the input-transform chain; not the batch of a foreign model
        and not the returned audio.  An unknown name is refused here (ValueError); validate=False hands an integer to the
        library as it is (it refuses what is outside the contract and keeps the previous setting)."""
        from . import codec as K
        kind = K.kind_of(codec) if validate else int(codec)
        N.check(self._L.fb_set_codec(self._h, C.c_int(kind)))
        self.codec = K.name_of(kind)

    def debug_codec(self, kind, audio_list):
        """k_codec on rows handed in as they are (fb_debug_codec): kind as set_codec names it (not None), int16 utterances of
        any length >= 1; a list of int16 arrays.  The engine's own codec setting is neither read nor changed."""
        from . import codec as K
        lst = [np.ascontiguousarray(a, np.int16).reshape(-1) for a in audio_list]
        off = np.zeros(len(lst) + 1, np.int64)
        off[1:] = np.cumsum([a.size for a in lst])
        cat = np.ascontiguousarray(np.concatenate(lst))
        out = np.empty_like(cat)
        N.check(self._L.fb_debug_codec(self._h, C.c_int(K.kind_of(kind)), N.ptr(cat), N.ptr(off), C.c_int(len(lst)), N.ptr(out)))
        return [out[off[i]:off[i + 1]].copy() for i in range(len(lst))]

    def set_eot(self, r):
        """Expectation over transformation (fb_set_eot): get_grad and attack score every NES sample under r independent draws
        of a randomised victim (a noise stage in the chain, dither > 0) and average the losses and scores before the
        gradient estimate and the stop test.  1 (the default) changes nothing; 2 .. 32."""
        r = int(r)
        if not 1 <= r <= 32:
            raise ValueError("EOT size %d outside 1 .. 32" % r)
        N.check(self._L.fb_set_eot(self._h, C.c_int(r)))
        self.eot = r

    def set_companions(self, wavs, bits_per_sample=16):
        """Companion utterances (fb_set_companions): get_grad and attack then search for ONE perturbation over K = K1 + 1
        utterances -- the audio of the call and these --, the losses and scores averaged over them (and over the EOT draws)
        before the gradient estimate and the stop test.  wavs: an int16 array (K1, N) or a list of float / int16 utterances
        of equal length N, the length of the audio the calls will attack; None (or an empty list) clears them.  ValueError for
        unequal lengths, more than 31 companions or K * eot > 32.  The stop test reads the MEAN loss: see
        FakeBob.attack(companions=...) for per-utterance results."""
        from .companions import MAX_REPLICAS, as_companions
        arr = as_companions(wavs, None, bits_per_sample)
        if arr is None:
            N.check(self._L.fb_set_companions(self._h, None, C.c_int(0), C.c_int64(0)))
            self.companions = None
            return
        if (arr.shape[0] + 1) * self.eot > MAX_REPLICAS:
            raise ValueError("%d utterances under eot %d: utterances * eot is at most %d" % (arr.shape[0] + 1, self.eot, MAX_REPLICAS))
        N.check(self._L.fb_set_companions(self._h, N.ptr(arr), C.c_int(arr.shape[0]), C.c_int64(arr.shape[1])))
        self.companions = arr

    def set_query_eot(self, quorum):
        """Voted decisions (fb_set_query_eot): with a quorum set attack_pso, attack_kenansville and attack_hsj accept
        set_eot(r) and companions -- every candidate row is scored r' = K * eot times, PSO reads the mean loss, the two
        decision-only attacks the number of adversarial replicas (the row's vote) against the quorum.  None (the default)
        switches it off: the three attacks refuse EOT and companions.  "majority" (or -1): r' // 2 + 1 votes; 1 .. 32: that
        many (larger than r' is refused at the attack call)."""
        from .query_eot import quorum_code
        q = quorum_code(quorum)
        N.check(self._L.fb_set_query_eot(self._h, C.c_int(q)))
        self.query_eot = None if q == 0 else ("majority" if q == -1 else q)

    @property
    def query_replicas(self):
        """r' of the three query attacks: K * eot replicas of every candidate row under set_query_eot, else 1"""
        if self.query_eot is None:
            return 1
        return (1 + (0 if self.companions is None else self.companions.shape[0])) * self.eot

    def _vote_args(self, raw, tv, task, attack_type, label):
        raw = np.ascontiguousarray(raw, np.float64)
        if raw.ndim != 3:
            raise ValueError("raw must be (rows, replicas, n_out)")
        rows, r, _m = raw.shape
        tv = np.ascontiguousarray(tv, np.int32).reshape(-1)
        if tv.size != rows * r:
            raise ValueError("tv must hold rows * replicas entries")
        S = max(self.n_speakers, 1)
        head = (self._h, N.ptr(raw), N.ptr(tv), C.c_int(rows), C.c_int(r), C.c_int(N.TASK[task]))
        tail = (C.c_int(N.ATTACK[attack_type]), C.c_int(int(label)))
        return raw, tv, rows, S, head, tail

    def debug_vote(self, raw, tv, task, threshold, attack_type, label):
        """k_vote alone (fb_debug_vote) on raw scores (rows, replicas, n_out) of the loaded system and tv (rows * replicas)
        -> votes (rows,), nodec (rows,) int32 and mean (rows, S) float64."""
        raw, tv, rows, S, head, tail = self._vote_args(raw, tv, task, attack_type, label)
        votes, nodec = np.empty(rows, np.int32), np.empty(rows, np.int32)
        mean = np.empty((rows, S), np.float64)
        N.check(self._L.fb_debug_vote(*head, C.c_double(float(threshold)), *tail, N.ptr(votes), N.ptr(nodec), N.ptr(mean)))
        return votes, nodec, mean

    def bench_vote(self, raw, tv, task, threshold, attack_type, label, reps=50):
        """Milliseconds per k_vote launch (fb_bench_vote: device events around `reps` launches)."""
        raw, tv, rows, S, head, tail = self._vote_args(raw, tv, task, attack_type, label)
        ms = C.c_double()
        N.check(self._L.fb_bench_vote(*head, C.c_double(float(threshold)), *tail, C.c_int(int(reps)), C.byref(ms)))
        return ms.value

    # ---- foreign victims of the swarm and the decision-only attacks: the two launches alone
    def debug_rows_to_model(self, rows_i16, bits_per_sample=16, dtype=np.float64):
        """k_rows_to_model alone (fb_debug_rows_to_model): int16 rows (rows, N) -> (rows, N) float32 / float64, the audio a
        foreign model reads."""
        q = np.ascontiguousarray(rows_i16, np.int16)
        q = q.reshape(1, -1) if q.ndim == 1 else q
        dt = np.dtype(dtype)
        out = np.empty(q.shape, dt)
        N.check(self._L.fb_debug_rows_to_model(self._h, N.ptr(q), C.c_int(q.shape[0]), C.c_int64(q.shape[1]),
                                               C.c_int(int(bits_per_sample)), C.c_int(self._np_dt(dt)), N.ptr(out)))
        return out

    def debug_decide_foreign(self, scores, task, threshold):
        """k_decide_foreign alone (fb_debug_decide_foreign): scores (rows, S) float32 / float64 -> (decisions (rows,) int32,
        scores (rows, S) float64), the two parts of the look block."""
        sc = np.ascontiguousarray(scores)
        if sc.dtype not in (np.float32, np.float64):
            sc = sc.astype(np.float64)
        rows, S = sc.shape
        dec, out = np.empty(rows, np.int32), np.empty((rows, S), np.float64)
        N.check(self._L.fb_debug_decide_foreign(self._h, N.ptr(sc), C.c_int(self._np_dt(sc.dtype)), C.c_int(rows), C.c_int(S),
                                                C.c_int(N.TASK[task]), C.c_double(float(threshold)), N.ptr(dec), N.ptr(out)))
        return dec, out

    @staticmethod
    def _np_dt(dt):
        return N.FB_DT_F32 if np.dtype(dt) == np.float32 else N.FB_DT_F64

    def bench_foreign_rows(self, rows, n, S=1, bits_per_sample=16, reps=20):
        """fb_bench_foreign_rows -> milliseconds: k_rows_to_model<float>, k_rows_to_model<double>, k_decide_foreign per
        launch; the float64 rows copied to the host; the int16 rows copied and widened on the host."""
        ms = np.zeros(5, np.float64)
        N.check(self._L.fb_bench_foreign_rows(self._h, C.c_int(int(rows)), C.c_int64(int(n)), C.c_int(int(bits_per_sample)),
                                              C.c_int(int(S)), C.c_int(int(reps)), N.ptr(ms)))
        return dict(rows_f32=float(ms[0]), rows_f64=float(ms[1]), decide=float(ms[2]), d2h_f64=float(ms[3]),
                    d2h_i16_widen=float(ms[4]))

    def debug_compose(self, q, a0, r, seed, stream, epoch):
        """The int16 rows the composing launch writes (fb_debug_compose) for the hand-made NES rows q (B, N) and the cast
        original a0 (N,), r draws per utterance at (seed, stream, epoch): an array (B, K, r, N), K - 1 the companions set."""
        q = np.ascontiguousarray(q, np.int16)
        q = q.reshape(1, -1) if q.ndim == 1 else q
        a0 = np.ascontiguousarray(a0, np.int16).reshape(-1)
        B, n = q.shape
        if a0.size != n:
            raise ValueError("a0 of %d samples, rows of %d" % (a0.size, n))
        K = 1 if self.companions is None else self.companions.shape[0] + 1
        out = np.empty((B, K, int(r), n), np.int16)
        N.check(self._L.fb_debug_compose(self._h, N.ptr(q), C.c_int(B), C.c_int64(n), N.ptr(a0), C.c_int(int(r)),
                                         C.c_uint64(int(seed)), C.c_uint32(int(stream)), C.c_uint32(int(epoch)), N.ptr(out)))
        return out

    def set_feature_compression(self, ratio, iters=10):
        """Feature compression (fb_set_feature_compression; SpeakerGuard's FeCo): the engine clusters the voiced feature rows
        of every utterance it scores with k-means -- keyed initialisation, `iters` Lloyd iterations -- and scores the
        max(1, floor(T * ratio)) centres in the frames' place.  0 < ratio <= 1, iters 1 .. 64; ratio None switches it off.
        Not applied to foreign models, to enrolment statistics or to debug_mfcc / debug_feats."""
        if ratio is None:
            N.check(self._L.fb_set_feature_compression(self._h, C.c_double(0.0), C.c_int(0)))
            self.feature_compression = None
            return
        N.check(self._L.fb_set_feature_compression(self._h, C.c_double(float(ratio)), C.c_int(int(iters))))
        self.feature_compression = (float(ratio), int(iters))

    def debug_feature_compress(self, mats, r, seed, stream, epoch):
        """k_feature_compress on feature matrices handed in as they are (fb_debug_feature_compress): `mats`, a list of B
        float32 arrays (T_b, feat_dim), T_b = 0 allowed, each scored under r replicas at (seed, stream, epoch) of the contract
        -> a list of B lists of r arrays (k_b, feat_dim)."""
        D, r = self.feat_dim, int(r)
        lst = [np.ascontiguousarray(m, np.float32).reshape(-1, D) for m in mats]
        rep = [m for m in lst for _ in range(r)]
        off = np.zeros(len(rep) + 1, np.int32)
        off[1:] = np.cumsum([m.shape[0] for m in rep])
        cat = np.ascontiguousarray(np.concatenate(rep, axis=0))
        out = np.empty_like(cat)
        out_off = np.empty_like(off)
        N.check(self._L.fb_debug_feature_compress(self._h, N.ptr(cat), N.ptr(off), C.c_int(len(lst)), C.c_int(r),
                                                  C.c_uint64(int(seed)), C.c_uint32(int(stream)), C.c_uint32(int(epoch)),
                                                  N.ptr(out), N.ptr(out_off)))
        return [[out[out_off[b * r + j]:out_off[b * r + j + 1]].copy() for j in range(r)] for b in range(len(lst))]

    def debug_feature_compress_vjp(self, mats, r, seed, stream, epoch, cots):
        """debug_feature_compress with the kernel's keep outputs on, then k_wb_feco_t on float64 cotangents handed in
        (fb_debug_feature_compress_vjp): `cots`, a list of B lists of r arrays (k_b, feat_dim), k_b = max(1, floor(T_b * ratio))
        (0 rows for T_b = 0) -> (labels, counts, xbar): lists of B lists of r arrays, int32 (T_b,), int32 (k_b,) and float64
        (T_b, feat_dim) = cots[label] / counts[label]."""
        D, r = self.feat_dim, int(r)
        lst = [np.ascontiguousarray(m, np.float32).reshape(-1, D) for m in mats]
        rep = [m for m in lst for _ in range(r)]
        off = np.zeros(len(rep) + 1, np.int32)
        off[1:] = np.cumsum([m.shape[0] for m in rep])
        cat = np.ascontiguousarray(np.concatenate(rep, axis=0))
        crep = [np.ascontiguousarray(cots[b][j], np.float64).reshape(-1, D) for b in range(len(lst)) for j in range(r)]
        ccat = np.ascontiguousarray(np.concatenate(crep, axis=0)) if crep else np.zeros((0, D), np.float64)
        out_off = np.empty_like(off)
        labels = np.full(cat.shape[0], -1, np.int32)
        counts = np.zeros(max(ccat.shape[0], 1), np.int32)
        xbar = np.zeros(cat.shape, np.float64)
        N.check(self._L.fb_debug_feature_compress_vjp(self._h, N.ptr(cat), N.ptr(off), C.c_int(len(lst)), C.c_int(r),
                                                      C.c_uint64(int(seed)), C.c_uint32(int(stream)), C.c_uint32(int(epoch)),
                                                      N.ptr(ccat if ccat.size else np.zeros((1, D), np.float64)),
                                                      C.c_int(ccat.shape[0]), N.ptr(out_off), N.ptr(labels), N.ptr(counts),
                                                      N.ptr(xbar)))
        for R, c in enumerate(crep):
            if out_off[R + 1] - out_off[R] != c.shape[0]:
                raise ValueError("row %d: %d cotangent rows for %d centres" % (R, c.shape[0], out_off[R + 1] - out_off[R]))
        rows = range(len(lst))
        return ([[labels[off[b * r + j]:off[b * r + j + 1]].copy() for j in range(r)] for b in rows],
                [[counts[out_off[b * r + j]:out_off[b * r + j + 1]].copy() for j in range(r)] for b in rows],
                [[xbar[off[b * r + j]:off[b * r + j + 1]].copy() for j in range(r)] for b in rows])

    def debug_feco_keys(self, seed, stream, epoch, utt, replica, T):
        """The uint32 initialisation keys of frames 0 .. T - 1 of (utterance row `utt`, replica) (fb_debug_feco_keys)."""
        keys = np.empty(int(T), np.uint32)
        N.check(self._L.fb_debug_feco_keys(self._h, C.c_uint64(int(seed)), C.c_uint32(int(stream)), C.c_uint32(int(epoch)),
                                           C.c_uint32(int(utt)), C.c_int(int(replica)), C.c_int(int(T)), N.ptr(keys)))
        return keys

    def debug_tf_noise(self, seed, stream, epoch, utt, replica, stage, i0, n):
        """The float32 normals a noise stage at position `stage` adds to samples i0 .. i0 + n - 1 (fb_debug_tf_noise)."""
        z = np.empty(int(n), np.float32)
        N.check(self._L.fb_debug_tf_noise(self._h, C.c_uint64(int(seed)), C.c_uint32(int(stream)), C.c_uint32(int(epoch)),
                                          C.c_uint32(int(utt)), C.c_int(int(replica)), C.c_int(int(stage)),
                                          C.c_int64(int(i0)), C.c_int64(int(n)), N.ptr(z)))
        return z

    def debug_input_transform_eot(self, audio_list, r, seed, stream, epoch):
        """The replicated int16 batch the MFCC would read at (seed, stream, epoch) of the noise contract
        (fb_debug_input_transform_eot): a list of len(audio_list) lists of r arrays."""
        lst = [np.ascontiguousarray(a, np.int16).reshape(-1) for a in audio_list]
        off = np.zeros(len(lst) + 1, np.int64)
        off[1:] = np.cumsum([a.size for a in lst])
        cat = np.ascontiguousarray(np.concatenate(lst))
        out = np.empty(cat.size * int(r), np.int16)
        N.check(self._L.fb_debug_input_transform_eot(self._h, N.ptr(cat), N.ptr(off), C.c_int(len(lst)), C.c_int(int(r)),
                                                     C.c_uint64(int(seed)), C.c_uint32(int(stream)), C.c_uint32(int(epoch)),
                                                     N.ptr(out)))
        res, o = [], 0
        for a in lst:
            res.append([out[o + j * a.size:o + (j + 1) * a.size].copy() for j in range(int(r))])
            o += a.size * int(r)
        return res

    @property
    def feat_dim(self):
        return self.cfg.num_ceps * (self.cfg.delta_order + 1)

    def load_gmm(self, models):
        self.load_gmm_arrays(*stack_models(models))

    def load_gmm_arrays(self, gc, miv, iv):
        """gconsts (M, C), means_invvars (M, C, D), inv_vars (M, C, D), float32 -- Kaldi's DiagGmm members."""
        gc, miv, iv = (np.ascontiguousarray(a, np.float32) for a in (gc, miv, iv))
        M, Cn, D = miv.shape
        N.check(self._L.fb_load_gmm(self._h, C.c_int(M), C.c_int(Cn), C.c_int(D), N.ptr(gc),
                                    N.ptr(miv), N.ptr(iv)))
        self.n_models = M
        self._gmm_shape = (Cn, D)
        self.task = "OSI"
        self.kind = "gmm"

    def load_ivector(self, system, task="OSI"):
        """system: models.IvectorSystem"""
        sy, keep = N.ivector_struct(system)
        self._iv_nsel = system.num_gselect
        self._iv_shape = (system.C, system.D, system.R, system.S)
        N.check(self._L.fb_load_ivector(self._h, C.byref(sy), C.c_int(N.TASK[task])))
        self.n_models = system.S
        self.task = task
        self.kind = "iv"

    def load_xvector(self, system, task="OSI"):
        """system: models.XvectorSystem"""
        sy, keep = N.xvector_struct(system)
        N.check(self._L.fb_load_xvector(self._h, C.byref(sy), C.c_int(N.TASK[task])))
        self._xv_shape = ([ly["W"].shape[0] for ly in system.layers], system.P, system.R)
        self.n_models = system.S
        self.task = task
        self.kind = "xv"

    def debug_xv_embed(self, mats, layer):
        """The loaded x-vector system's chain on feature rows handed in (fb_debug_xv_embed): `mats`, a list of (T_b,
        feat_dim) float32 arrays -> that frame layer's outputs, a list of (T_b, dout) float32 arrays (layer < n_layers);
        the pooled statistics, (B, 2 P) float64 (layer == n_layers); the embeddings, (B, R) float64 (n_layers + 1)."""
        douts, P, R = self._xv_shape
        lst = [np.ascontiguousarray(m, np.float32).reshape(-1, self.feat_dim) for m in mats]
        off = np.zeros(len(lst) + 1, np.int32)
        off[1:] = np.cumsum([m.shape[0] for m in lst])
        cat = np.ascontiguousarray(np.concatenate(lst, axis=0))
        layer = int(layer)
        if layer < len(douts):
            out = np.empty((cat.shape[0], douts[max(layer, 0)]), np.float32)
        else:
            out = np.empty((len(lst), 2 * P if layer == len(douts) else R), np.float64)
        N.check(self._L.fb_debug_xv_embed(self._h, N.ptr(cat), N.ptr(off), C.c_int(len(lst)), C.c_int(layer), N.ptr(out)))
        if layer < len(douts):
            return [out[off[b]:off[b + 1]].copy() for b in range(len(lst))]
        return out

    def debug_xv_backward(self, mats, ebar, stage):
        """The loaded x-vector system's chain on feature rows handed in, then the TDNN's backward from the embedding cotangents
        ebar (B, R) down to `stage` (fb_debug_xv_backward): n_layers + 1 -> the cotangent on the statistics, (B, 2 P) float64;
        n_layers -> on the last frame layer's output, a list of (T_b, P) float32; 1 .. n_layers - 1 -> on the input of that
        layer, a list of (T_b, din) float32; 0 -> on the feature rows, a list of (T_b, feat_dim) float64."""
        douts, P, R = self._xv_shape
        lst = [np.ascontiguousarray(m, np.float32).reshape(-1, self.feat_dim) for m in mats]
        off = np.zeros(len(lst) + 1, np.int32)
        off[1:] = np.cumsum([m.shape[0] for m in lst])
        cat = np.ascontiguousarray(np.concatenate(lst, axis=0))
        ebar = np.ascontiguousarray(ebar, np.float64).reshape(len(lst), R)
        stage, nl = int(stage), len(douts)
        if stage > nl:
            out = np.empty((len(lst), 2 * P), np.float64)
        elif stage <= 0:
            out = np.empty((cat.shape[0], self.feat_dim), np.float64)
        else:
            out = np.empty((cat.shape[0], douts[stage - 1]), np.float32)
        N.check(self._L.fb_debug_xv_backward(self._h, N.ptr(cat), N.ptr(off), C.c_int(len(lst)), N.ptr(ebar), C.c_int(stage), N.ptr(out),
                                             C.c_int64(out.nbytes)))
        if stage > nl:
            return out
        return [out[off[b]:off[b + 1]].copy() for b in range(len(lst))]

    def debug_xv_masks(self, layer):
        """The ReLU decisions of frame layer `layer` for the batch scored last with them kept -- a white-box call on an x-vector
        system, or debug_xv_backward (fb_debug_xv_masks) -> (rows, dout) uint8, 1 where the layer's float32 z was > 0."""
        douts, _P, _R = self._xv_shape
        size = C.c_int64()
        N.check(self._L.fb_debug_xv_masks(self._h, C.c_int(int(layer)), None, C.c_int64(0), C.byref(size)))
        out = np.empty(size.value, np.uint8)
        N.check(self._L.fb_debug_xv_masks(self._h, C.c_int(int(layer)), N.ptr(out), C.c_int64(out.nbytes), C.byref(size)))
        return out.reshape(-1, douts[int(layer)])

    def debug_wb_xv_route(self):
        """Launches of the TDNN backward the last white-box call (or debug_xv_backward) enqueued (fb_debug_wb_xv_route): a dict
        backend_t, segment_t, pool_t, act_t, affine_t, unsplice -- the last three once per frame layer."""
        info = (C.c_int * 6)()
        N.check(self._L.fb_debug_wb_xv_route(self._h, info))
        return dict(zip(("backend_t", "segment_t", "pool_t", "act_t", "affine_t", "unsplice"), [int(v) for v in info]))

    def bench_xvector(self, B, T, reps=10, seed=0):
        """fb_bench_xvector on B utterances of T seeded feature rows each -> a dict of milliseconds per launch: rowmax and
        affine (one entry per frame layer), pool, segment, backend."""
        douts, _P, _R = self._xv_shape
        rng = np.random.default_rng(seed)
        cat = (3.0 * rng.standard_normal((B * T, self.feat_dim), dtype=np.float32))
        off = (np.arange(B + 1, dtype=np.int64) * T).astype(np.int32)
        rm, af, tail = np.zeros(len(douts)), np.zeros(len(douts)), np.zeros(3)
        N.check(self._L.fb_bench_xvector(self._h, N.ptr(cat), N.ptr(off), C.c_int(B), C.c_int(int(reps)), N.ptr(rm), N.ptr(af), N.ptr(tail)))
        return dict(rowmax=rm.tolist(), affine=af.tolist(), pool=float(tail[0]), segment=float(tail[1]), backend=float(tail[2]))

    def bench_xv_backward(self, B, T, reps=10, seed=0):
        """fb_bench_xv_backward on B utterances of T seeded feature rows each -> a dict of milliseconds per launch of the TDNN
        backward: act_t, affine_t and unsplice (one entry per frame layer), segment_t, pool_t."""
        douts, _P, _R = self._xv_shape
        rng = np.random.default_rng(seed)
        cat = (3.0 * rng.standard_normal((B * T, self.feat_dim), dtype=np.float32))
        off = (np.arange(B + 1, dtype=np.int64) * T).astype(np.int32)
        ac, af, us, tail = np.zeros(len(douts)), np.zeros(len(douts)), np.zeros(len(douts)), np.zeros(2)
        N.check(self._L.fb_bench_xv_backward(self._h, N.ptr(cat), N.ptr(off), C.c_int(B), C.c_int(int(reps)), N.ptr(ac), N.ptr(af), N.ptr(us),
                                             N.ptr(tail)))
        return dict(act_t=ac.tolist(), affine_t=af.tolist(), unsplice=us.tolist(), segment_t=float(tail[0]), pool_t=float(tail[1]))

    def gmm_acc_stats(self, wav):
        """UBM (loaded alone) posterior statistics of one utterance: occ[C], F[C,D] (float64), voiced frames."""
        wav = np.ascontiguousarray(wav).reshape(-1)
        if wav.dtype != np.int16:
            raise TypeError("gmm_acc_stats takes int16 samples")
        Cn, D = self._gmm_shape
        occ = np.empty(Cn, np.float64)
        F = np.empty((Cn, D), np.float64)
        tv = C.c_int()
        N.check(self._L.fb_gmm_acc_stats(self._h, N.ptr(wav), C.c_int64(wav.size), N.ptr(occ), N.ptr(F), C.byref(tv)))
        return occ, F, tv.value

    def last_ivectors(self, B, R):
        """i-vectors (B, R) of the batch scored last with an i-vector system."""
        out = np.empty((B, R), np.float64)
        N.check(self._L.fb_last_ivectors(self._h, C.c_int(B), N.ptr(out)))
        return out

    debug_ivectors = last_ivectors   # name the parity tests use

    @property
    def gmm_kernel(self):
        """'fx2' | 'bx3': the diagonal-GMM arithmetic the loaded model runs on (fb_gmm_kernel_mode)."""
        rc = self._L.fb_gmm_kernel_mode(self._h)
        if rc < 0:
            N.check(rc)
        return {1: "bx3", 2: "fx2"}[rc]

    @property
    def gmm_kernel_variant(self):
        """The kernel the loaded GMM system is scored with: 'bx3', 'fx2', or 'fx2w/P' -- the one-wave-per-SIMD
        kernel with the speaker models as deltas from model 0, P = 1 .. 3 partial products per delta item
        (fb_gmm_kernel_variant)."""
        rc = self._L.fb_gmm_kernel_variant(self._h, None)
        if rc < 0:
            N.check(rc)
        return {1: "bx3", 2: "fx2"}.get(rc) or "fx2w/%d" % (rc - 10)

    @property
    def gmm_delta_tiles(self):
        """(tiles with 1, 2, 3 partial products per K chunk in their delta items): k_gmm_fx2w's per-tile choice for the
        loaded model (fb_gmm_delta_tiles); (0, 0, 0) when another kernel scores it."""
        a, b, c = C.c_int(), C.c_int(), C.c_int()
        rc = self._L.fb_gmm_delta_tiles(self._h, C.byref(a), C.byref(b), C.byref(c))
        if rc < 0:
            N.check(rc)
        return (a.value, b.value, c.value)

    @property
    def gmm_delta_tiles_f6(self):
        """Tiles of the F6 class (corrections as block-scaled fp6 products, fb_gmm_delta_tiles_f6)."""
        rc = self._L.fb_gmm_delta_tiles_f6(self._h)
        if rc < 0:
            N.check(rc)
        return rc

    @property
    def gmm_shift_rms(self):
        """fb_load_gmm's measure of how far the models were adapted from model 0 (what P is chosen from)."""
        v = C.c_double()
        rc = self._L.fb_gmm_kernel_variant(self._h, C.byref(v))
        if rc < 0:
            N.check(rc)
        return v.value

    def debug_iv_active(self):
        n = C.c_int()
        N.check(self._L.fb_debug_iv_active(self._h, C.byref(n)))
        return n.value

    def debug_iv_gselect(self, rows_cap=None):
        """(sel[rows][num_gselect], info dict) of the last i-vector batch -- fb_debug_iv_gselect."""
        info = (C.c_int64 * 6)()
        N.check(self._L.fb_debug_iv_gselect(self._h, None, C.c_int64(0), info))
        rows, nsel = int(info[4]), int(self._iv_nsel)
        sel = np.empty((rows, nsel), np.int32)
        N.check(self._L.fb_debug_iv_gselect(self._h, N.ptr(sel), C.c_int64(sel.size), info))
        return sel, dict(threshold_path=bool(info[0]), path=int(info[0]), overflow=int(info[1]), max_list=int(info[2]),
                         survivors=int(info[3]), rows=rows, chunks=int(info[5]))

    # fb_debug_frontend_route's codes (include/fakebob_hip_test.h: FB_ROUTE_*)
    _ROUTE_MFCC = {0: None, 1: "k_mfcc_f32<12>", 2: "k_mfcc_f32<0>", 3: "k_mfcc_r16<12,true>", 4: "k_mfcc_r16<12,false>",
                   5: "k_mfcc_r16<0,true>", 6: "k_mfcc_r16<0,false>", 7: "k_mfcc",
                   # the dithered forms (cfg.dither > 0)
                   8: "k_mfcc_f32<12,dither>", 9: "k_mfcc_f32<0,dither>", 10: "k_mfcc_r16<12,true,dither>",
                   11: "k_mfcc_r16<12,false,dither>", 12: "k_mfcc_r16<0,true,dither>", 13: "k_mfcc_r16<0,false,dither>",
                   14: "k_mfcc<dither>"}
    _ROUTE_CHAIN = {0: None, 1: "split", 2: "whole", 3: "vad+delta_cmvn", 4: "separate", 5: "separate+sliding"}
    _ROUTE_CM = {0: None, 1: "fused", 2: "registers", 3: "lds", 4: "global"}

    def debug_frontend_route(self):
        """What the front end of the last batch ran (fb_debug_frontend_route): a dict of mfcc (the kernel), chain (the
        VAD / deltas / CMVN launches), compress (where the CompressedMatrix round trip ran, None when it is off), t_max
        (the longest utterance, frames) and B."""
        info = (C.c_int * 5)()
        N.check(self._L.fb_debug_frontend_route(self._h, info))
        return dict(mfcc=self._ROUTE_MFCC[info[0]], chain=self._ROUTE_CHAIN[info[1]], compress=self._ROUTE_CM[info[2]],
                    t_max=int(info[3]), B=int(info[4]))

    # fb_debug_launch_shape's GMM kernel codes (include/fakebob_hip_test.h: FB_SHAPE_GMM_*)
    _SHAPE_GMM = {0: None, 1: "fx2w", 2: "fx2", 3: "bx3"}

    def debug_launch_shape(self):
        """The launch geometry of the last batch as the launchers chose it (fb_debug_launch_shape): a dict of gmm (the
        kernel, None when none ran), n_chunks, sub (chunks per k_gmm_fx2w workgroup), grid_chunks, xcd_map (0: the plain
        2-D grid), passes, strips, tiles_min / tiles_max (component tiles of a chunk), k_mfcc_f32's cus, rounds and
        blocks (0 when another MFCC kernel ran), and up_threads: the threads per workgroup of the update launch that
        followed the batch inside an attack (0: none did)."""
        info = (C.c_int * 13)()
        N.check(self._L.fb_debug_launch_shape(self._h, info))
        keys = ("n_chunks", "sub", "grid_chunks", "xcd_map", "passes", "strips", "tiles_min", "tiles_max", "cus", "rounds", "blocks",
                "up_threads")
        d = dict(gmm=self._SHAPE_GMM[info[0]])
        d.update((k, int(v)) for k, v in zip(keys, info[1:]))
        return d

    def set_system(self, task, z_mean=None, z_std=None):
        zm = None if z_mean is None else np.ascontiguousarray(z_mean, np.float64)
        zs = None if z_std is None else np.ascontiguousarray(z_std, np.float64)
        N.check(self._L.fb_set_system(self._h, C.c_int(N.TASK[task]),
                                      None if zm is None else N.ptr(zm),
                                      None if zs is None else N.ptr(zs)))
        self.task = task

    @property
    def n_speakers(self):
        return self._L.fb_num_speakers(self._h)

    # ---- scoring
    def score_raw(self, audio_list, bits_per_sample=16):
        """list of 1-D arrays (int16, or float in [-1,1]) -> raw[B,M], tv[B]."""
        B = len(audio_list)
        off = np.zeros(B + 1, np.int64)
        off[1:] = np.cumsum([a.size for a in audio_list])
        raw = np.empty((B, self.n_models), np.float64)
        tv = np.empty(B, np.int32)
        if all(a.dtype == np.int16 for a in audio_list):
            cat = np.ascontiguousarray(np.concatenate([a.reshape(-1) for a in audio_list]))
            N.check(self._L.fb_score_i16(self._h, N.ptr(cat), N.ptr(off), C.c_int(B), N.ptr(raw), N.ptr(tv)))
        else:
            # mixed / float input: int16 entries are exact in float64 after /2^(bits-1)
            scale = float(2 ** (bits_per_sample - 1))
            parts = [a.reshape(-1).astype(np.float64) / scale if a.dtype == np.int16
                     else a.reshape(-1).astype(np.float64) for a in audio_list]
            cat = np.ascontiguousarray(np.concatenate(parts))
            N.check(self._L.fb_score_f64(self._h, N.ptr(cat), N.ptr(off), C.c_int(B),
                                         C.c_int(bits_per_sample), N.ptr(raw), N.ptr(tv)))
        return raw, tv

    def system_scores(self, raw):
        raw = np.ascontiguousarray(raw, np.float64)
        B = raw.shape[0]
        out = np.empty((B, self.n_speakers), np.float64)
        N.check(self._L.fb_system_scores(self._h, N.ptr(raw), C.c_int(B), N.ptr(out)))
        return out

    # ---- NES
    def get_grad(self, params, audio, it=0, noise_pos=None, want_grad=True):
        return self._get_grad("fb_get_grad", params, max(self.n_speakers, 1), audio, it, noise_pos, want_grad)

    def attack(self, params, audio, noise_all=None):
        return self._attack("fb_attack", params, self.n_speakers, audio, noise_all)

    def _nes_call(self, fn, err, *args):
        try:
            N.check(getattr(self._L, fn)(*args))
        except N.NativeError as ex:
            self._raise_cb(err, ex)

    def _get_grad(self, fn, params, n_scores, audio, it, noise_pos, want_grad=True, model=None):
        """The get_grad* wrappers: model(n) -> (the arguments between params and audio, the callback's error cell) for
        a foreign model, None for this engine's system."""
        audio = np.ascontiguousarray(audio, np.float64).reshape(-1)
        n = audio.size
        npz = None if noise_pos is None else np.ascontiguousarray(noise_pos, np.float64)
        if npz is not None and npz.shape != (n, params.samples_per_draw // 2):
            raise ValueError("noise_pos must be (N, samples_per_draw//2)")
        mid, err = model(n) if model else ((), [None])
        grad = np.empty(n, np.float64) if want_grad else None
        fl, al = C.c_double(), C.c_double()
        sc = np.empty(n_scores, np.float64)
        self._nes_call(fn, err, self._h, C.byref(params), *mid, N.ptr(audio), C.c_int64(n), C.c_uint32(it),
                       None if npz is None else N.ptr(npz), C.byref(fl), None if grad is None else N.ptr(grad),
                       C.byref(al), N.ptr(sc))
        return fl.value, grad, al.value, sc

    def _attack(self, fn, params, S, audio, noise_all, model=None):
        """The attack* wrappers -> (int16 adv, flag, float64 adv, trace); model as in _get_grad."""
        audio = np.ascontiguousarray(audio, np.float64).reshape(-1)
        n = audio.size
        na = None if noise_all is None else np.ascontiguousarray(noise_all, np.float64)
        mid, err = model(n) if model else ((), [None])
        adv = np.empty(n, np.int16)
        adv_f = np.empty(n, np.float64)
        trace = np.zeros((max(params.max_iter, 1), 3 + S), np.float64)
        nt, flag = C.c_int(), C.c_int()
        self._nes_call(fn, err, self._h, C.byref(params), *mid, N.ptr(audio), C.c_int64(n),
                       None if na is None else N.ptr(na), N.ptr(adv), N.ptr(adv_f), N.ptr(trace), C.byref(nt),
                       C.byref(flag))
        return adv, flag.value, adv_f, trace[:nt.value]

    # ---- white-box gradients (GMM-UBM systems on an undefended victim)
    def set_wb_bpda(self, on):
        """fb_set_wb_bpda: with True, get_grad_wb and attack_wb differentiate through an input-transform chain, a codec and
        the replicas of set_eot -- BPDA through the non-differentiable stages, EOT over the random ones (the derivative rules
        are in include/fakebob_hip.h).  False (as created): every defence is refused and nothing else changes."""
        N.check(self._L.fb_set_wb_bpda(self._h, C.c_int(1 if on else 0)))
        self.wb_bpda = bool(on)

    def set_wb_ivector(self, on):
        """fb_set_wb_ivector: with True, get_grad_wb and attack_wb differentiate through a loaded i-vector-PLDA system (the
        selection and the pruned set held constant: the rules are in include/fakebob_hip.h).  False (as created): an
        i-vector system is refused and nothing else changes; a GMM-UBM system runs the same launches either way."""
        N.check(self._L.fb_set_wb_ivector(self._h, C.c_int(1 if on is True else 0 if on is False else int(on))))
        self.wb_ivector = bool(on)

    def set_wb_xvector(self, on):
        """fb_set_wb_xvector: with True, get_grad_wb, attack_wb, attack_cw2 and attack_psy differentiate through a loaded
        x-vector (TDNN) system -- the forward's ReLU and pooling-floor decisions held constant: the rules are in
        include/fakebob_hip.h --, undefended, or with set_wb_bpda(True) through a chain, a codec and set_eot(r).  An air channel,
        dither, companions and a play offset stay refused.  False (as created): an x-vector system is refused and nothing else
        changes; the other kinds run the same launches either way."""
        N.check(self._L.fb_set_wb_xvector(self._h, C.c_int(1 if on is True else 0 if on is False else int(on))))
        self.wb_xvector = bool(on)

    def set_wb_air(self, on):
        """fb_set_wb_air: with True, get_grad_wb and attack_wb differentiate through the over-the-air channel of
        set_air_channel -- the forward's own drawn responses transposed, a saturated output passing zero; with set_eot(r) the
        EOT-over-rooms gradient (the rules are in include/fakebob_hip.h).  A chain, a codec and r > 1 still need
        set_wb_bpda(True), an i-vector system set_wb_ivector(True).  False (as created): a channel is refused and nothing else
        changes.  0 / 1 and booleans only; anything else is handed to the library, which refuses it."""
        N.check(self._L.fb_set_wb_air(self._h, C.c_int(1 if on is True else 0 if on is False else int(on))))
        self.wb_air = bool(on)

    def set_wb_frontend(self, on):
        """fb_set_wb_frontend: with True, get_grad_wb and attack_wb differentiate through feature compression (the forward's
        final k-means assignment held constant: a centre is the mean of its members) and through Kaldi's dither (the forward's
        draws, redrawn as constants); the rules are in include/fakebob_hip.h.  Neither needs another switch at r = 1; a chain, a
        codec and r > 1 still need set_wb_bpda(True), an air channel set_wb_air(True), an i-vector system set_wb_ivector(True).
        False (as created): both are refused and nothing else changes.  0 / 1 and booleans only; anything else is handed to
        the library, which refuses it."""
        N.check(self._L.fb_set_wb_frontend(self._h, C.c_int(1 if on is True else 0 if on is False else int(on))))
        self.wb_frontend = bool(on)

    def set_wb_universal(self, on):
        """fb_set_wb_universal: with True, get_grad_wb and attack_wb accept the companions of set_companions on a GMM-UBM
        system: the exact gradient of the loss averaged over the K utterances one perturbation is scored on, through the
        composition's clip (a clipped sample passes zero; the rules are in include/fakebob_hip.h).  Companions need no other
        switch at eot = 1; a chain, a codec and r > 1 still need set_wb_bpda(True), an air channel set_wb_air(True), feature
        compression and dither set_wb_frontend(True).  False (as created): companions are refused and nothing else changes.
        0 / 1 and booleans only; anything else is handed to the library, which refuses it."""
        N.check(self._L.fb_set_wb_universal(self._h, C.c_int(1 if on is True else 0 if on is False else int(on))))
        self.wb_universal = bool(on)

    def debug_wb_universal_route(self):
        """k_wb_compose_t launches of the last get_grad_wb / attack_wb / debug_wb_compose_t call
        (fb_debug_wb_universal_route): one per iteration with companions set, none without."""
        n = C.c_int(0)
        N.check(self._L.fb_debug_wb_universal_route(self._h, C.byref(n)))
        return int(n.value)

    def debug_wb_compose_t(self, cot, q, a0, comp, eot=1):
        """k_wb_compose_t alone (fb_debug_wb_compose_t): float64 cotangents (K * eot, n), int16 q (n,), a0 (n,) and companions
        (K - 1, n) -> grad (n,) float64: the replicas' cotangents summed, rho ascending, a companion's clipped samples masked."""
        q = np.ascontiguousarray(q, np.int16).reshape(-1)
        a0 = np.ascontiguousarray(a0, np.int16).reshape(-1)
        n = q.size
        comp = np.ascontiguousarray(comp, np.int16).reshape(-1, n) if comp is not None and np.size(comp) else None
        K = 1 if comp is None else comp.shape[0] + 1
        cot = np.ascontiguousarray(cot, np.float64).reshape(K * int(eot), n)
        if a0.size != n:
            raise ValueError("a0 has %d samples, q %d" % (a0.size, n))
        grad = np.empty(n, np.float64)
        N.check(self._L.fb_debug_wb_compose_t(self._h, N.ptr(cot), N.ptr(q), N.ptr(a0), None if comp is None else N.ptr(comp),
                                              C.c_int(K), C.c_int(int(eot)), C.c_int64(n), N.ptr(grad)))
        return grad

    def set_play_offset(self, S):
        """Play offset (fb_set_play_offset): get_grad and attack -- and, under set_wb_universal(True), get_grad_wb and attack_wb
        -- then score every replica of every row with the perturbation rotated circularly by an offset of its own, uniform in
        0 .. S: the loudspeaker plays the perturbation on a loop and cannot time it to the victim's speech.  None or 0 (the
        default) clears it and changes nothing; up to 2 ** 31 - 2, and below the length of the audio the calls attack.  The
        stop test reads the MEAN loss over the offsets: see FakeBob.attack(...)'s per_offset for what each offset does."""
        from .play_offset import MAX_OFFSET
        S = 0 if S is None else int(S)
        if not 0 <= S <= MAX_OFFSET:
            raise ValueError("play offset %d outside 0 .. 2^31 - 2" % S)
        N.check(self._L.fb_set_play_offset(self._h, C.c_int64(S)))
        self.play_offset = S

    def debug_play_offsets(self, seed, stream, epoch, B, r, utt0=0):
        """The offsets k_play_compose draws (fb_debug_play_offsets) for B rows from utterance row utt0 on and r replicas of
        each, at (seed, stream, epoch) under the S set: a uint32 array (B, r)."""
        tau = np.empty((int(B), int(r)), np.uint32)
        N.check(self._L.fb_debug_play_offsets(self._h, C.c_uint64(int(seed)), C.c_uint32(int(stream)), C.c_uint32(int(epoch)),
                                              C.c_uint32(int(utt0)), C.c_int(int(B)), C.c_int(int(r)), N.ptr(tau)))
        return tau

    def debug_play_route(self):
        """k_play_compose launches since the last set_play_offset call (fb_debug_play_route)."""
        n = C.c_int(0)
        N.check(self._L.fb_debug_play_route(self._h, C.byref(n)))
        return int(n.value)

    def bench_play_compose(self, B, n, eot, reps=50, K=1):
        """Milliseconds per k_play_compose launch on B rows of n samples, K utterances per row and eot draws of each
        (fb_bench_play_compose: device events around `reps` launches)."""
        ms = C.c_double()
        N.check(self._L.fb_bench_play_compose(self._h, C.c_int(int(B)), C.c_int64(int(n)), C.c_int(int(K)), C.c_int(int(eot)),
                                              C.c_int(int(reps)), C.byref(ms)))
        return ms.value

    def debug_wb_play_route(self):
        """k_wb_play_compose_t launches of the last get_grad_wb / attack_wb / debug_wb_play_compose_t call
        (fb_debug_wb_play_route): one per iteration with a play offset set, none without."""
        n = C.c_int(0)
        N.check(self._L.fb_debug_wb_play_route(self._h, C.byref(n)))
        return int(n.value)

    def debug_wb_play_compose_t(self, cot, q, a0, comp, tau, eot=1):
        """k_wb_play_compose_t alone (fb_debug_wb_play_compose_t): debug_wb_compose_t's arguments and the offsets tau (K * eot,),
        every one below n -> grad (n,) float64 by the "Transposed rule" of the play offset."""
        q = np.ascontiguousarray(q, np.int16).reshape(-1)
        a0 = np.ascontiguousarray(a0, np.int16).reshape(-1)
        n = q.size
        comp = np.ascontiguousarray(comp, np.int16).reshape(-1, n) if comp is not None and np.size(comp) else None
        K = 1 if comp is None else comp.shape[0] + 1
        cot = np.ascontiguousarray(cot, np.float64).reshape(K * int(eot), n)
        tau = np.ascontiguousarray(tau, np.uint32).reshape(K * int(eot))
        if a0.size != n:
            raise ValueError("a0 has %d samples, q %d" % (a0.size, n))
        grad = np.empty(n, np.float64)
        N.check(self._L.fb_debug_wb_play_compose_t(self._h, N.ptr(cot), N.ptr(q), N.ptr(a0), None if comp is None else N.ptr(comp),
                                                   N.ptr(tau), C.c_int(K), C.c_int(int(eot)), C.c_int64(n), N.ptr(grad)))
        return grad

    def debug_wb_feco_route(self):
        """k_wb_feco_t launches of the last get_grad_wb / attack_wb / debug_feature_compress_vjp call
        (fb_debug_wb_feco_route): r per iteration with feature compression on, none otherwise."""
        n = C.c_int(0)
        N.check(self._L.fb_debug_wb_feco_route(self._h, C.byref(n)))
        return int(n.value)

    def debug_wb_feco_state(self, j=0, cap=1 << 16):
        """What the forward of the last get_grad_wb call kept of replica j's feature compression (fb_debug_wb_feco_state; read
        it before any other scoring call) -> (labels (Tv,) int32, counts (k,) int32)."""
        labels, counts = np.empty(int(cap), np.int32), np.empty(int(cap), np.int32)
        tv, k = C.c_int(0), C.c_int(0)
        N.check(self._L.fb_debug_wb_feco_state(self._h, C.c_int(int(j)), C.c_int(int(cap)), N.ptr(labels), N.ptr(counts),
                                               C.byref(tv), C.byref(k)))
        return labels[:tv.value].copy(), counts[:k.value].copy()

    def debug_air_conv_t(self, taps, cot, sat=None):
        """k_air_conv_t alone (fb_debug_air_conv_t): int16 taps (B, L) -- or (L,) for one row --, float64 cotangents (B, n) and
        (optional) saturation bytes (B, n) -> dx (B, n) float64 = 2^-14 * the correlation of the masked cotangent with the
        row's taps, all rows in one launch."""
        taps = np.ascontiguousarray(taps, np.int16)
        taps = taps.reshape(1, -1) if taps.ndim == 1 else taps
        cot = np.ascontiguousarray(cot, np.float64)
        cot = cot.reshape(1, -1) if cot.ndim == 1 else cot
        if cot.shape[0] != taps.shape[0]:
            raise ValueError("%d responses for %d rows" % (taps.shape[0], cot.shape[0]))
        if sat is not None:
            sat = np.ascontiguousarray(sat, np.uint8).reshape(cot.shape)
        dx = np.empty_like(cot)
        N.check(self._L.fb_debug_air_conv_t(self._h, N.ptr(taps), C.c_int(taps.shape[0]), C.c_int(taps.shape[1]),
                                            C.c_int64(cot.shape[1]), N.ptr(cot), None if sat is None else N.ptr(sat), N.ptr(dx)))
        return dx

    def debug_air_conv_t_chunk(self):
        """Samples of dx one workgroup of k_air_conv_t computes (fb_debug_air_conv_t_chunk)."""
        return int(self._L.fb_debug_air_conv_t_chunk())

    def debug_wb_air_route(self):
        """k_air_conv_t launches of the last get_grad_wb / attack_wb / debug_defence_vjp / debug_air_conv_t call
        (fb_debug_wb_air_route): one per iteration whatever the EOT size, none without a channel."""
        n = C.c_int(0)
        N.check(self._L.fb_debug_wb_air_route(self._h, C.byref(n)))
        return int(n.value)

    def get_grad_wb(self, params, audio, want_grad=True):
        """fb_get_grad_wb: get_grad_wb_iter at iter = 0."""
        return self.get_grad_wb_iter(params, audio, 0, want_grad)

    def get_grad_wb_iter(self, params, audio, iter=0, want_grad=True):
        """fb_get_grad_wb_iter: the analytic gradient of the loss at `audio` -> (grad (N,) float64 = d loss / d audio, in the
        units of get_grad's estimate; adver_loss; score0 (S,)).  adver_loss and score0 are get_grad's own: the same forward.
        samples_per_draw and sigma are not read; seed, stream and `iter` (the epoch of the draws, as get_grad's `it`) key the
        random stages of a defended victim.  Refused (NativeError, FB_E_STATE) for i-vector systems and while an air channel,
        feature compression, dither or companions are set; an input transform, a codec and EOT only after set_wb_bpda(True).
        After set_wb_ivector(True) an i-vector system is differentiated as well (never with set_eot > 1); after
        set_wb_xvector(True) an x-vector system is (undefended, or with set_wb_bpda(True) through a chain, a codec and EOT); after
        set_wb_air(True) an air channel is too (the forward's drawn responses transposed); after set_wb_frontend(True) feature
        compression and dither are (the forward's final assignment and its dither draws held constant); after
        set_wb_universal(True) companions are: the gradient of the mean loss over the K utterances, a_0 of the composition being
        the cast of `audio` itself (get_grad_wb_from: a_0 given)."""
        return self.get_grad_wb_from(params, audio, None, iter, want_grad)

    def get_grad_wb_from(self, params, audio, original=None, iter=0, want_grad=True):
        """fb_get_grad_wb_from: get_grad_wb_iter with a_0 of the composition given (set_wb_universal, set_companions): original
        (None: audio itself, the call is then fb_get_grad_wb_iter) is the audio whose int16 cast is a_0, as the attack's start
        is in attack_wb -- audio - original is the perturbation the companions carry -- and, under set_play_offset, the loop that is rotated on every
        replica, utterance 0's included.  With neither companions nor a play offset it is not read."""
        audio = np.ascontiguousarray(audio, np.float64).reshape(-1)
        n = audio.size
        grad = np.empty(n, np.float64) if want_grad else None
        al = C.c_double()
        sc = np.empty(max(self.n_speakers, 1), np.float64)
        if original is None:
            N.check(self._L.fb_get_grad_wb_iter(self._h, C.byref(params), N.ptr(audio), C.c_int64(n), C.c_int(int(iter)), C.byref(al),
                                                None if grad is None else N.ptr(grad), N.ptr(sc)))
            return grad, al.value, sc
        original = np.ascontiguousarray(original, np.float64).reshape(-1)
        if original.size != n:
            raise ValueError("original has %d samples, audio %d" % (original.size, n))
        N.check(self._L.fb_get_grad_wb_from(self._h, C.byref(params), N.ptr(audio), N.ptr(original), C.c_int64(n), C.c_int(int(iter)),
                                            C.byref(al), None if grad is None else N.ptr(grad), N.ptr(sc)))
        return grad, al.value, sc

    def attack_wb(self, params, audio):
        """fb_attack_wb: FakeBob.attack's loop with the analytic gradient in place of the NES estimate (momentum = 0: PGD
        with the margin loss; max_iter = 1: the single-step attack) -> (int16 adv, flag, float64 adv, trace), as attack.
        GMM-UBM systems; i-vector systems after set_wb_ivector(True) and x-vector systems after set_wb_xvector(True), with the
        same loop, trace layout and stop test."""
        audio = np.ascontiguousarray(audio, np.float64).reshape(-1)
        n, S = audio.size, max(self.n_speakers, 1)
        adv = np.empty(n, np.int16)
        adv_f = np.empty(n, np.float64)
        trace = np.zeros((max(params.max_iter, 1), 3 + S), np.float64)
        nt, flag = C.c_int(), C.c_int()
        N.check(self._L.fb_attack_wb(self._h, C.byref(params), N.ptr(audio), C.c_int64(n), N.ptr(adv), N.ptr(adv_f),
                                     N.ptr(trace), C.byref(nt), C.byref(flag)))
        return adv, flag.value, adv_f, trace[:nt.value]

    def attack_cw2(self, params, cw2, audio):
        """fb_attack_cw2: Carlini-Wagner's L2 attack on the analytic gradient (tanh space, Adam, a binary search over the
        constant; fakebob_hip.h, "CW2") -> dict(adv (N,) int16, success +-1, adver_f64 (N,), trace (rows, 3 + S) of
        {l2, adver_loss, c, score0}, rows_per_step (search_steps,), best_l2, const).  params.max_iter counts the iterations of
        ONE search step.  Victims as attack_wb takes them, except companions, an air channel, feature compression and dither,
        which are refused whatever the switches say."""
        return self._tanh_attack(self._L.fb_attack_cw2, params, cw2, [], audio, 3, [("best_l2", C.c_double)])

    def _tanh_attack(self, fn, params, cw2, extra, audio, width, best):
        """What attack_cw2 and attack_psy marshal: fn(handle, params, cw2, *extra, audio, N, adv, adver_f64, trace, n_trace,
        rows_per_step, success, *best, const).  width: the trace columns in front of the scores; best: (key, ctypes type) of the
        attack's own results, in the order of the call."""
        audio = np.ascontiguousarray(audio, np.float64).reshape(-1)
        n, S = audio.size, max(self.n_speakers, 1)
        steps = int(cw2.search_steps)
        total = max(steps, 0) * max(int(params.max_iter), 0)
        if not 1 <= steps <= 32 or total > 2 ** 30:   # (the library says which; nothing of that size is allocated for it here)
            total = 1
        adv = np.empty(n, np.int16)
        adv_f = np.empty(n, np.float64)
        trace = np.zeros((max(total, 1), width + S), np.float64)
        per = np.zeros(32, np.int32)
        nt, flag, cc = C.c_int(), C.c_int(), C.c_double()
        cells = [(key, ctype()) for key, ctype in best]
        N.check(fn(self._h, C.byref(params), C.byref(cw2), *(extra + [N.ptr(audio), C.c_int64(n), N.ptr(adv), N.ptr(adv_f), N.ptr(trace),
                                                                       C.byref(nt), N.ptr(per), C.byref(flag)] +
                                                             [C.byref(c) for _key, c in cells] + [C.byref(cc)])))
        out = dict(adv=adv, success=flag.value, adver_f64=adv_f, trace=trace[:nt.value].copy(), rows_per_step=per[:steps].copy())
        out.update((key, c.value) for key, c in cells)
        out["const"] = cc.value
        return out

    def debug_cw2_step(self, cw2, g, x, a0, w0, mod, m1, m2, adver_loss, c, gbest_l2, t, p1, p2):
        """One k_cw2_ctl + k_cw2_step pair on arrays handed in (fb_debug_cw2_step) -> dict(mod, m1, m2, x_next, l2, l2_next,
        gate, take, best_row, best_x).  No system has to be loaded."""
        return self._tanh_step(self._L.fb_debug_cw2_step, "debug_cw2_step: the seven arrays", [C.byref(cw2)], (g, x, a0, w0, mod, m1, m2),
                               [C.c_double(adver_loss), C.c_double(c), C.c_double(gbest_l2), C.c_int(int(t)), C.c_double(p1),
                                C.c_double(p2)], ["l2"])

    def _tanh_step(self, fn, what, head, arrays, scalars, now):
        """What debug_cw2_step and debug_psy_step marshal: fn(handle, *head, N, *arrays, *scalars, mod, m1, m2, x_next, *now,
        l2_next, gate, take, best_row, best_x).  now: the keys of the float64 results k_*_ctl left, in the order of the call."""
        arrs = [np.ascontiguousarray(a, np.float64).reshape(-1) for a in arrays]
        n = arrs[0].size
        if any(a.size != n for a in arrs):
            raise ValueError("%s must have one length" % what)
        out = [np.empty(n, np.float64) for _ in range(4)]
        best_row, best_x = np.empty(n, np.int16), np.empty(n, np.float64)
        cells = [C.c_double() for _ in now]
        l2n, gate, take = C.c_double(), C.c_int(), C.c_int()
        N.check(fn(self._h, *(head + [C.c_int64(n)] + [N.ptr(a) for a in arrs] + scalars + [N.ptr(o) for o in out] +
                              [C.byref(c) for c in cells] + [C.byref(l2n), C.byref(gate), C.byref(take), N.ptr(best_row), N.ptr(best_x)])))
        res = dict(mod=out[0], m1=out[1], m2=out[2], x_next=out[3])
        res.update(zip(now, (c.value for c in cells)))
        res.update(l2_next=l2n.value, gate=gate.value, take=take.value, best_row=best_row, best_x=best_x)
        return res

    def attack_psy(self, params, cw2, psy, audio):
        """fb_attack_psy: attack_cw2's loop with the psychoacoustic masking distortion D(delta) + l2_weight * l2 (fakebob_hip.h,
        "masking") -> dict(adv (N,) int16, success +-1, adver_f64 (N,), trace (rows, 5 + S) of {dist, l2, n_over, adver_loss, c,
        score0}, rows_per_step (search_steps,), best_dist, best_l2, n_over, const).  psy: psy_params(theta, psd_max, ...)."""
        return self._tanh_attack(self._L.fb_attack_psy, params, cw2, [C.byref(psy)], audio, 5,
                                 [("best_dist", C.c_double), ("best_l2", C.c_double), ("n_over", C.c_int)])

    def debug_psy_loss(self, psy, delta, want_P=False):
        """The masking loss and its gradient at a perturbation handed in (fb_debug_psy_loss) -> dict(D, n_over, gd (N,), P [F, K]
        or None).  No system has to be loaded."""
        delta = np.ascontiguousarray(delta, np.float64).reshape(-1)
        n = delta.size
        gd = np.empty(n, np.float64)
        P = np.empty((max(int(psy.n_frames), 1), max(int(psy.window), 0) // 2 + 1), np.float64) if want_P else None
        D, no = C.c_double(), C.c_int()
        N.check(self._L.fb_debug_psy_loss(self._h, C.byref(psy), C.c_int64(n), N.ptr(delta), C.byref(D), C.byref(no), N.ptr(gd),
                                          N.ptr(P) if want_P else None))
        return dict(D=D.value, n_over=no.value, gd=gd, P=P)

    def debug_psy_step(self, cw2, l2_weight, g, gd, x, a0, w0, mod, m1, m2, adver_loss, c, D, n_over, gbest_dist, t, p1, p2):
        """One k_psy_ctl + k_psy_step pair on arrays handed in (fb_debug_psy_step) -> dict(mod, m1, m2, x_next, l2, dist, l2_next,
        gate, take, best_row, best_x).  No system has to be loaded."""
        return self._tanh_step(self._L.fb_debug_psy_step, "debug_psy_step: the eight arrays", [C.byref(cw2), C.c_double(l2_weight)],
                               (g, gd, x, a0, w0, mod, m1, m2),
                               [C.c_double(adver_loss), C.c_double(c), C.c_double(D), C.c_int(int(n_over)), C.c_double(gbest_dist),
                                C.c_int(int(t)), C.c_double(p1), C.c_double(p2)], ["l2", "dist"])

    def debug_defence_vjp(self, wav, cot, seed=0, stream=0, iter=0):
        """The defences' transposes alone (fb_debug_defence_vjp): wav (n,) int16, cot (r, n) float64 on the rows the front
        end would read, r = the engine's EOT size -> (dwav (r, n) float64, out (r, n) int16 = those rows)."""
        wav = np.ascontiguousarray(wav, np.int16).reshape(-1)
        r = int(getattr(self, "eot", 1))
        cot = np.ascontiguousarray(cot, np.float64).reshape(r, wav.size)
        dwav = np.empty((r, wav.size), np.float64)
        out = np.empty((r, wav.size), np.int16)
        N.check(self._L.fb_debug_defence_vjp(self._h, N.ptr(wav), C.c_int64(wav.size), C.c_uint64(int(seed)), C.c_uint32(int(stream)),
                                             C.c_int(int(iter)), N.ptr(cot), N.ptr(dwav), N.ptr(out)))
        return dwav, out

    def debug_wb_route(self):
        """Launches of the white-box backward the last get_grad_wb / attack_wb / debug_defence_vjp call enqueued
        (fb_debug_wb_route): a dict ctl, ctl_rep, backward, chain_t; with an i-vector system loaded also iv_ctl,
        iv_backend_t, iv_solve, iv_stats_t, iv_post_t (all zero for a GMM-UBM system, and left out for one)."""
        info = (C.c_int * 9)()
        N.check(self._L.fb_debug_wb_route(self._h, info))
        names = ("ctl", "ctl_rep", "backward", "chain_t", "iv_ctl", "iv_backend_t", "iv_solve", "iv_stats_t", "iv_post_t")
        return dict(list(zip(names, [int(v) for v in info]))[:9 if getattr(self, "kind", None) == "iv" else 4])

    def debug_iv_backend_grad(self, ivec, w):
        """k_wb_iv_backend_t alone (fb_debug_iv_backend_grad): ivec (R,), w (S,) -> (R,) float64, the gradient of
        sum_s w[s] * LLR_s (raw, before the z-norm) with respect to the i-vector."""
        if getattr(self, "kind", None) != "iv":
            raise ValueError("debug_iv_backend_grad needs a loaded i-vector system")
        Cn, D, R, S = self._iv_shape
        ivec = np.ascontiguousarray(ivec, np.float64).reshape(-1)
        w = np.ascontiguousarray(w, np.float64).reshape(-1)
        if ivec.size != R or w.size != S:
            raise ValueError("debug_iv_backend_grad takes an i-vector of %d and %d weights" % (R, S))
        out = np.empty(R, np.float64)
        N.check(self._L.fb_debug_iv_backend_grad(self._h, N.ptr(ivec), N.ptr(w), N.ptr(out)))
        return out

    def debug_iv_feat_grad(self, feats, cot):
        """The extractor's backward alone (fb_debug_iv_feat_grad): feats (Tv, D) float32 handed in as they are, cot (R,) a
        cotangent on the i-vector -> (Tv, D) float64 = d <cot, ivec(feats)> / d feats.  debug_iv_gselect and last_ivectors
        afterwards describe the forward it ran."""
        if getattr(self, "kind", None) != "iv":
            raise ValueError("debug_iv_feat_grad needs a loaded i-vector system")
        Cn, D, R, S = self._iv_shape
        feats = np.ascontiguousarray(feats, np.float32)
        cot = np.ascontiguousarray(cot, np.float64).reshape(-1)
        if feats.ndim != 2 or feats.shape[1] != D or feats.shape[0] < 1 or cot.size != R:
            raise ValueError("debug_iv_feat_grad takes rows of %d features and a cotangent of %d" % (D, R))
        out = np.empty(feats.shape, np.float64)
        N.check(self._L.fb_debug_iv_feat_grad(self._h, N.ptr(feats), C.c_int(feats.shape[0]), N.ptr(cot), N.ptr(out)))
        return out

    def debug_gmm_feat_grad(self, feats, w):
        """The GMM backward alone (fb_debug_gmm_feat_grad): feats (Tv, D) float32 handed in as they are, w (M,) the
        weights d loss / d raw[m] -> (Tv, D) float64."""
        feats = np.ascontiguousarray(feats, np.float32)
        w = np.ascontiguousarray(w, np.float64).reshape(-1)
        Cn, D = self._gmm_shape
        if feats.ndim != 2 or feats.shape[1] != D or w.size != self.n_models:
            raise ValueError("debug_gmm_feat_grad takes rows of %d features and %d weights" % (D, self.n_models))
        out = np.empty(feats.shape, np.float64)
        N.check(self._L.fb_debug_gmm_feat_grad(self._h, N.ptr(feats), C.c_int(feats.shape[0]), N.ptr(w), N.ptr(out)))
        return out

    def debug_frontend_vjp(self, wav, cot):
        """The front-end backward alone (fb_debug_frontend_vjp): int16 samples and a cotangent (Tv, feat_dim) on the
        compacted voiced rows -> (dwav (n,) float64 in int16 units, the voiced mask (T,) bool the backward used)."""
        wav = np.ascontiguousarray(wav, np.int16).reshape(-1)
        cot = np.ascontiguousarray(cot, np.float64)
        dwav = np.empty(wav.size, np.float64)
        voiced = np.zeros(max(self._num_frames(wav.size), 1), np.uint8)
        N.check(self._L.fb_debug_frontend_vjp(self._h, N.ptr(wav), C.c_int64(wav.size), N.ptr(cot), N.ptr(dwav), N.ptr(voiced)))
        return dwav, voiced[:self._num_frames(wav.size)].astype(bool)

    # ---- particle swarm
    def attack_pso(self, params, pso, audio):
        """fb_attack_pso: the particle-swarm attack on this engine's system -> (int16 adv, flag, float64 adv, trace
        (n_iters, 3 + S): gbest loss, gbest particle, particles improved, gbest scores; losses (n_iters, P))."""
        return self._attack_pso(params, pso, audio, None)

    def attack_pso_foreign(self, params, pso, victim, audio):
        """fb_attack_pso_foreign: the same swarm, scored by a foreign model.  victim: a dict of mode ("host_scores" /
        "device_scores"), S, fn -- fn((N, B) float64) -> (B, S) scores, or fn(x [B, N] tensor) -> [B, S] on the GPU -- and,
        device mode, the torch tensors x [P, N] and scores [P, S] on this engine's device.  Returns what attack_pso does."""
        return self._attack_pso(params, pso, audio, victim)

    def _attack_pso(self, params, pso, audio, victim):
        audio = np.ascontiguousarray(audio, np.float64).reshape(-1)
        n, P = audio.size, max(int(pso.particles), 1)
        S = self.n_speakers if victim is None else max(int(victim["S"]), 1)
        adv = np.empty(n, np.int16)
        adv_f = np.empty(n, np.float64)
        rows = max(params.max_iter, 1)
        trace = np.zeros((rows, 3 + S), np.float64)
        losses = np.zeros((rows, P), np.float64)
        flag, ni = C.c_int(), C.c_int()
        tail = (N.ptr(audio), C.c_int64(n), N.ptr(adv), N.ptr(adv_f), C.byref(flag), C.byref(ni), N.ptr(trace), N.ptr(losses))
        if victim is None:
            N.check(self._L.fb_attack_pso(self._h, C.byref(params), C.byref(pso), *tail))
        else:
            self._foreign_call(self._L.fb_attack_pso_foreign, victim, P, n, (C.byref(params), C.byref(pso)), tail)
        return adv, flag.value, adv_f, trace[:ni.value], losses[:ni.value]

    def debug_pso_init(self, audio, epsilon, particles, v_max, seed, stream, bits_per_sample=16):
        """The swarm at t = 0 (fb_debug_pso_init) -> x, v (P, N) float64 and q (P, N) int16, the first batch."""
        audio = np.ascontiguousarray(audio, np.float64).reshape(-1)
        P = int(particles)
        shape = (max(P, 1), audio.size)
        x, v, q = np.empty(shape, np.float64), np.empty(shape, np.float64), np.empty(shape, np.int16)
        N.check(self._L.fb_debug_pso_init(self._h, N.ptr(audio), C.c_int64(audio.size), C.c_double(float(epsilon)), C.c_int(P),
                                          C.c_double(float(v_max)), C.c_uint64(int(seed)), C.c_uint32(int(stream)),
                                          C.c_int(int(bits_per_sample)), N.ptr(x), N.ptr(v), N.ptr(q)))
        return x, v, q

    def debug_pso_step(self, audio, epsilon, x, v, pb, gb, improved, g_new, w, c1, c2, v_max, seed, stream, t,
                       bits_per_sample=16):
        """One update of a swarm handed in as it is (fb_debug_pso_step): x, v, pb (P, N), gb (N,), improved (P,) flags,
        g_new the particle whose position becomes gb (-1: none) -> the new x, v, pb, gb and q, the int16 cast of the new x."""
        audio = np.ascontiguousarray(audio, np.float64).reshape(-1)
        x, v, pb = (np.ascontiguousarray(a, np.float64) for a in (x, v, pb))
        gb = np.ascontiguousarray(gb, np.float64).reshape(-1)
        P, n = x.shape
        if v.shape != (P, n) or pb.shape != (P, n) or gb.size != n or audio.size != n:
            raise ValueError("x, v, pb must be (P, N), gb and audio (N,)")
        imp = np.ascontiguousarray(improved, np.int32).reshape(-1)
        if imp.size != P:
            raise ValueError("improved must hold one flag per particle")
        xo, vo, po, go = np.empty_like(x), np.empty_like(v), np.empty_like(pb), np.empty_like(gb)
        q = np.empty((P, n), np.int16)
        N.check(self._L.fb_debug_pso_step(self._h, N.ptr(audio), C.c_int64(n), C.c_double(float(epsilon)), C.c_int(P), N.ptr(x),
                                          N.ptr(v), N.ptr(pb), N.ptr(gb), N.ptr(imp), C.c_int(int(g_new)), C.c_double(float(w)),
                                          C.c_double(float(c1)), C.c_double(float(c2)), C.c_double(float(v_max)),
                                          C.c_uint64(int(seed)), C.c_uint32(int(stream)), C.c_uint32(int(t)),
                                          C.c_int(int(bits_per_sample)), N.ptr(xo), N.ptr(vo), N.ptr(po), N.ptr(go), N.ptr(q)))
        return xo, vo, po, go, q

    # ---- decision-only attack
    def attack_kenansville(self, params, kv, audio, tables=None):
        """fb_attack_kenansville: the decision-only attack on this engine's system -> a dict: adv (int16), success (+-1),
        factor (-1: none), n_queries, and per round qs (n_rounds, G) (-1 in unused places), decisions (n_rounds, G) (-2: no
        voiced frames; unused places -3), scores (n_rounds, G, S) (unused places NaN), trace (n_rounds, 3) = lo, hi, rows.
        tables=None: fakebob_amd.kenansville.tables(kv.window)."""
        return self._attack_kenansville(params, kv, audio, tables, None)

    def attack_kenansville_foreign(self, params, kv, victim, audio, tables=None):
        """fb_attack_kenansville_foreign: the same search, the candidates decided by a foreign model.  victim: as for
        attack_pso_foreign, with mode "host_decisions" as well -- fn((N, B) float64) -> (decisions (B,), scores (B, S) or
        None); -2 is "no decision" -- and x [grid, N], scores [grid, S] in device mode.  Returns what attack_kenansville
        does; scores are the model's (NaN where a decision model gave none)."""
        return self._attack_kenansville(params, kv, audio, tables, victim)

    def _attack_kenansville(self, params, kv, audio, tables, victim):
        from . import kenansville as KV
        audio = np.ascontiguousarray(audio, np.float64).reshape(-1)
        n, S = audio.size, max(self.n_speakers if victim is None else int(victim["S"]), 1)
        G, R = min(max(int(kv.grid), 1), 64), min(max(int(kv.max_rounds), 1), 32)
        tab = self._kv_tables(KV, kv.window, tables)
        adv = np.empty(n, np.int16)
        qs = np.full((R, G), -1, np.int32)
        dec = np.full((R, G), -3, np.int32)
        sc = np.full((R, G, S), np.nan, np.float64)
        trace = np.zeros((R, 3), np.int32)
        flag, factor, nq, nr = C.c_int(), C.c_int(), C.c_int(), C.c_int()
        tail = (N.ptr(tab), N.ptr(audio), C.c_int64(n), N.ptr(adv), C.byref(flag), C.byref(factor), C.byref(nq), C.byref(nr),
                N.ptr(qs), N.ptr(dec), N.ptr(sc), N.ptr(trace))
        if victim is None:
            N.check(self._L.fb_attack_kenansville(self._h, C.byref(params), C.byref(kv), *tail))
        else:
            self._foreign_call(self._L.fb_attack_kenansville_foreign, victim, G, n, (C.byref(params), C.byref(kv)), tail)
        r = nr.value
        return dict(adv=adv, success=flag.value, factor=factor.value, n_queries=nq.value, qs=qs[:r], decisions=dec[:r],
                    scores=sc[:r], trace=trace[:r])

    @staticmethod
    def _kv_tables(KV, window, tables):
        """the four tables as one contiguous (4, W') int32 array: handed in as they are, or built for a window in range
        (a window out of range gets a dummy the library refuses by its own check)"""
        if tables is not None:
            return np.ascontiguousarray(tables, np.int32)
        W = int(window)
        return KV.tables(W) if KV.MIN_WINDOW <= W <= KV.MAX_WINDOW else np.zeros((4, 1), np.int32)

    def debug_kv_analyse(self, x, window, tables=None):
        """The analysis of int16 samples (fb_debug_kv_analyse) -> a, b (nw, K) int32, cum (nw, K) int64, E (nw,) int64."""
        from . import kenansville as KV
        x = np.ascontiguousarray(x, np.int16).reshape(-1)
        W = int(window)
        tab = self._kv_tables(KV, W, tables)
        nw, K = (-(-x.size // W), W // 2 + 1) if W > 0 else (1, 1)
        a, b = np.empty((nw, K), np.int32), np.empty((nw, K), np.int32)
        cum, E = np.empty((nw, K), np.int64), np.empty(nw, np.int64)
        N.check(self._L.fb_debug_kv_analyse(self._h, N.ptr(x), C.c_int64(x.size), C.c_int(W), N.ptr(tab), N.ptr(a), N.ptr(b),
                                            N.ptr(cum), N.ptr(E)))
        return a, b, cum, E

    def debug_kv_candidates(self, x, window, qs, tables=None):
        """The candidates of int16 samples for the factors qs (fb_debug_kv_candidates) -> y (rows, N) int16."""
        from . import kenansville as KV
        x = np.ascontiguousarray(x, np.int16).reshape(-1)
        q = np.ascontiguousarray(qs, np.int32).reshape(-1)
        tab = self._kv_tables(KV, window, tables)
        y = np.empty((max(q.size, 1), x.size), np.int16)
        N.check(self._L.fb_debug_kv_candidates(self._h, N.ptr(x), C.c_int64(x.size), C.c_int(int(window)), N.ptr(tab), N.ptr(q),
                                               C.c_int(q.size), N.ptr(y)))
        return y

    def bench_kv_kernels(self, x, window, qs, reps=50, tables=None):
        """Milliseconds per k_kv_analyse launch and per k_kv_candidates launch of len(qs) rows (fb_bench_kv_kernels: device
        events around `reps` launches of each)."""
        from . import kenansville as KV
        x = np.ascontiguousarray(x, np.int16).reshape(-1)
        q = np.ascontiguousarray(qs, np.int32).reshape(-1)
        tab = self._kv_tables(KV, window, tables)
        ms = np.zeros(2, np.float64)
        N.check(self._L.fb_bench_kv_kernels(self._h, N.ptr(x), C.c_int64(x.size), C.c_int(int(window)), N.ptr(tab), N.ptr(q),
                                            C.c_int(q.size), C.c_int(int(reps)), N.ptr(ms)))
        return float(ms[0]), float(ms[1])

    # ---- decision-only attack II: HopSkipJump
    def attack_hsj(self, params, hsj, audio, init, keep_x=False, log_capacity=None):
        """fb_attack_hsj: HopSkipJump on this engine's system, from `init` (decided as wanted) towards `audio` -> a dict: adv
        (int16, a row that was scored), adv_f64 (the boundary point x), success (+-1), dist2, n_iters, n_queries, trace
        (n_iters + 1, 8) = D2, B, n+, m, hi, rounds, queries so far, sigma (row 0: the start search), decisions (n_queries,)
        in scoring order (-2: no voiced frames) and, keep_x=True, xs (n_iters + 1, N): x after the start and every iteration.
        log_capacity=None: the decision log holds fb_hsj_max_rows entries."""
        return self._attack_hsj(params, hsj, audio, init, keep_x, log_capacity, None)

    def attack_hsj_foreign(self, params, hsj, victim, audio, init, keep_x=False, log_capacity=None):
        """fb_attack_hsj_foreign: the same walk, every row decided by a foreign model.  victim: as for
        attack_kenansville_foreign, with x [max(grid, num_evals_max), N] and scores [.., S] in device mode.  Returns what
        attack_hsj does (-2 in decisions: the model gave no decision)."""
        return self._attack_hsj(params, hsj, audio, init, keep_x, log_capacity, victim)

    def _attack_hsj(self, params, hsj, audio, init, keep_x, log_capacity, victim):
        audio = np.ascontiguousarray(audio, np.float64).reshape(-1)
        n = audio.size
        if init is not None:
            init = np.ascontiguousarray(init, np.float64).reshape(-1)
            if init.size != n:
                raise ValueError("init has %d samples, audio %d" % (init.size, n))
        T = max(int(params.max_iter), 0)
        cap = int(self._L.fb_hsj_max_rows(C.c_int(T), C.byref(hsj))) if log_capacity is None else int(log_capacity)
        dec = np.full(max(cap, 1), -3, np.int32)
        adv, adv_f = np.empty(n, np.int16), np.empty(n, np.float64)
        trace = np.zeros((T + 1, 8), np.float64)
        xs = np.zeros((T + 1, n), np.float64) if keep_x else None
        flag, ni, nq, d2 = C.c_int(), C.c_int(), C.c_int(), C.c_double()
        tail = (N.ptr(audio), N.ptr(init) if init is not None else None, C.c_int64(n), N.ptr(adv), N.ptr(adv_f), C.byref(flag),
                C.byref(d2), C.byref(ni), C.byref(nq), N.ptr(trace), N.ptr(dec), C.c_longlong(dec.size if cap >= 0 else -1),
                N.ptr(xs) if keep_x else None)
        if victim is None:
            N.check(self._L.fb_attack_hsj(self._h, C.byref(params), C.byref(hsj), *tail))
        else:
            rows_max = max(int(hsj.grid), int(hsj.num_evals_max), 1)
            self._foreign_call(self._L.fb_attack_hsj_foreign, victim, rows_max, n, (C.byref(params), C.byref(hsj)), tail)
        # (one log entry per candidate row; n_queries counts victim queries: under voted decisions r' = K * eot per row)
        n_log = nq.value // (self.query_replicas if victim is None else 1)
        res = dict(adv=adv, adv_f64=adv_f, success=flag.value, dist2=d2.value, n_iters=ni.value, n_queries=nq.value,
                   trace=trace[:ni.value + 1], decisions=dec[:n_log])
        if keep_x:
            res["xs"] = xs[:ni.value + 1] if flag.value == 1 else xs[:0]
        return res

    def debug_hsj_line(self, a, y, qs, bits_per_sample=16):
        """fb_debug_hsj_line -> rows (len(qs), N) int16 of line(y, q), and for qs[0] the adopt launch: x (N,) float64, D2."""
        a = np.ascontiguousarray(a, np.float64).reshape(-1)
        y = np.ascontiguousarray(y, np.float64).reshape(-1)
        if y.size != a.size:
            raise ValueError("a and y must have the same length")
        q = np.ascontiguousarray(qs, np.int32).reshape(-1)
        out = np.empty((max(q.size, 1), a.size), np.int16)
        x, d2 = np.empty(a.size, np.float64), C.c_double()
        N.check(self._L.fb_debug_hsj_line(self._h, N.ptr(a), N.ptr(y), C.c_int64(a.size), N.ptr(q), C.c_int(q.size),
                                          C.c_int(int(bits_per_sample)), N.ptr(out), N.ptr(x), C.byref(d2)))
        return out, x, d2.value

    def debug_hsj_probes(self, x, sigma, seed, stream, t, B, bits_per_sample=16):
        """fb_debug_hsj_probes -> the B probe rows of x at iteration t, (B, N) int16."""
        x = np.ascontiguousarray(x, np.float64).reshape(-1)
        out = np.empty((max(int(B), 1), x.size), np.int16)
        N.check(self._L.fb_debug_hsj_probes(self._h, N.ptr(x), C.c_int64(x.size), C.c_double(float(sigma)), C.c_uint64(int(seed)),
                                            C.c_uint32(int(stream)), C.c_uint32(int(t)), C.c_int(int(B)),
                                            C.c_int(int(bits_per_sample)), N.ptr(out)))
        return out

    def debug_hsj_dir(self, w, seed, stream, t, n):
        """fb_debug_hsj_dir -> v (n,) float64 = sum_j w_j z_j of iteration t, and S = ssq(v)."""
        w = np.ascontiguousarray(w, np.int32).reshape(-1)
        v, S = np.empty(int(n), np.float64), C.c_double()
        N.check(self._L.fb_debug_hsj_dir(self._h, N.ptr(w), C.c_int(w.size), C.c_uint64(int(seed)), C.c_uint32(int(stream)),
                                         C.c_uint32(int(t)), C.c_int64(int(n)), N.ptr(v), C.byref(S)))
        return v, S.value

    def debug_hsj_step(self, x, v, S, xi, G, bits_per_sample=16):
        """fb_debug_hsj_step -> the G step rows (G, N) int16 and y_m (G, N) float64."""
        x = np.ascontiguousarray(x, np.float64).reshape(-1)
        v = np.ascontiguousarray(v, np.float64).reshape(-1)
        if v.size != x.size:
            raise ValueError("x and v must have the same length")
        G = int(G)
        out, y = np.empty((max(G, 1), x.size), np.int16), np.empty((max(G, 1), x.size), np.float64)
        N.check(self._L.fb_debug_hsj_step(self._h, N.ptr(x), N.ptr(v), C.c_int64(x.size), C.c_double(float(S)), C.c_double(float(xi)),
                                          C.c_int(G), C.c_int(int(bits_per_sample)), N.ptr(out), N.ptr(y)))
        return out, y

    def bench_hsj_kernels(self, a, y, B, G=15, reps=20, bits_per_sample=16):
        """Milliseconds per launch (fb_bench_hsj_kernels: device events around `reps` launches of each) -> a dict: line, adopt,
        probes, probes_keep, dir_draw, dir_kept, step, nes_batch (k_perturb of 2 ceil(B / 2) + 1 rows)."""
        a = np.ascontiguousarray(a, np.float64).reshape(-1)
        y = np.ascontiguousarray(y, np.float64).reshape(-1)
        ms = np.zeros(8, np.float64)
        N.check(self._L.fb_bench_hsj_kernels(self._h, N.ptr(a), N.ptr(y), C.c_int64(a.size), C.c_int(int(B)), C.c_int(int(G)),
                                             C.c_int(int(bits_per_sample)), C.c_int(int(reps)), N.ptr(ms)))
        return dict(zip(("line", "adopt", "probes", "probes_keep", "dir_draw", "dir_kept", "step", "nes_batch"), ms.tolist()))

    def attack_iter_seconds(self, n):
        """Seconds per iteration of the last attack / attack_ext (device clock, fb_attack_iter_seconds); of the last
        attack_pso, per round of the last attack_kenansville and per iteration of the last attack_hsj (entry 0: its start
        search), as the host measured them."""
        out = np.zeros(max(int(n), 0), np.float64)
        if n > 0:
            N.check(self._L.fb_attack_iter_seconds(self._h, N.ptr(out), C.c_int(int(n))))
        return out

    # ---- NES with a foreign model (the reference's plugin API): scores come from `score_fn`
    @staticmethod
    def _score_cb(score_fn, S, err):
        """score_fn(audios (N, B) float64) -> (B, S) scores, wrapped as an fb_score_cb.  The model gets its OWN
        C-contiguous (N, B) array, as the reference hands it one (FAKEBOB.py:237): the callback's buffer is the
        engine's pinned staging area, recycled on the next iteration, and a model may keep or edit its batch.  An
        exception raised by the model is kept in err[0] and re-raised by the caller (a ctypes callback cannot
        propagate it)."""
        def _cb(_ctx, aud, n, b, out):
            try:
                # (N, B) copy, columns = utterances (np.array: ascontiguousarray hands back a view of the buffer when n == 1)
                a = np.array(np.ctypeslib.as_array(aud, shape=(b, n)).T, order="C")
                sc = np.asarray(score_fn(a), np.float64).reshape(b, S)
                np.ctypeslib.as_array(out, shape=(b, S))[...] = sc
                return 0
            except BaseException as ex:  # noqa: BLE001
                err[0] = ex
                return 1
        return N.SCORE_CB(_cb)

    @staticmethod
    def _raise_cb(err, ex):
        if getattr(ex, "code", None) == N.FB_E_CALLBACK and err[0] is not None:
            raise err[0]
        raise ex

    @staticmethod
    def _decide_cb(decide_fn, S, err):
        """decide_fn(audios (N, B) float64) -> (decisions (B,), scores (B, S) or None), wrapped as an fb_decide_cb.  The model
        gets its OWN C-contiguous (N, B) array, as _score_cb hands it one; scores it does not give stay NaN."""
        def _cb(_ctx, aud, n, b, dec, out):
            try:
                a = np.array(np.ctypeslib.as_array(aud, shape=(b, n)).T, order="C")
                d, sc = decide_fn(a)
                np.ctypeslib.as_array(dec, shape=(b,))[...] = np.asarray(d).reshape(b)
                if sc is not None:
                    np.ctypeslib.as_array(out, shape=(b, S))[...] = np.asarray(sc, np.float64).reshape(b, S)
                return 0
            except BaseException as ex:  # noqa: BLE001
                err[0] = ex
                return 1
        return N.DECIDE_CB(_cb)

    _VICTIM_MODES = {"host_scores": N.FB_VICTIM_HOST_SCORES, "host_decisions": N.FB_VICTIM_HOST_DECISIONS,
                     "device_scores": N.FB_VICTIM_DEVICE_SCORES}

    def _foreign_call(self, fn, victim, rows_max, n, head, tail):
        """fn(engine, *head, fb_victim, *tail) for the victim dict of attack_*_foreign; a mode the library does not know
        (an int) is handed through for it to refuse.  An exception raised by the model is re-raised here.  check_extent=False
        in a device victim leaves the size of x and scores to the library's own check of the allocations."""
        mode = victim["mode"]
        S, err = int(victim["S"]), [None]
        v = N.Victim()
        v.mode, v.S = self._VICTIM_MODES.get(mode, mode if isinstance(mode, int) else 0), S
        keep = []
        if mode == "host_scores" and victim.get("fn") is not None:
            v.score = self._score_cb(victim["fn"], S, err)
        elif mode == "host_decisions" and victim.get("fn") is not None:
            v.decide = self._decide_cb(victim["fn"], S, err)
        elif mode == "device_scores" and victim.get("fn") is not None:
            x, scores = victim["x"], victim["scores"]
            m = self._dev_buffers(rows_max, S, n, x, scores, 0, exact=victim.get("check_extent", True))
            keep.append(m)
            v.dev = C.pointer(m)
            v.score_dev = self._score_dev_cb(victim["fn"], x, scores, S, err)
        try:
            N.check(fn(self._h, *(tuple(head) + (C.byref(v),) + tuple(tail))))
        except N.NativeError as ex:
            self._raise_cb(err, ex)

    def _host_model(self, S, score_fn):
        def model(_n):
            err = [None]
            return (C.c_int(S), self._score_cb(score_fn, S, err), None), err
        return model

    def get_grad_ext(self, params, S, score_fn, audio, it=0, noise_pos=None):
        """fb_get_grad_ext: one NES gradient estimate at `audio` scored by score_fn."""
        return self._get_grad("fb_get_grad_ext", params, S, audio, it, noise_pos, model=self._host_model(S, score_fn))

    def attack_ext(self, params, S, score_fn, audio, noise_all=None):
        """fb_attack_ext: the whole attack loop with a foreign scorer -> (int16 adv, flag, float64 adv, trace)."""
        return self._attack("fb_attack_ext", params, S, audio, noise_all, model=self._host_model(S, score_fn))

    # ---- NES with a foreign model on the same GPU: the batch and the scores stay in device memory
    def _dev_model(self, params, S, n, x, scores, look_every):
        """fb_dev_model over the torch tensors x [B, N] and scores [B, S] (float32 / float64, on this engine's device)."""
        return self._dev_buffers(2 * (params.samples_per_draw // 2) + 1, S, n, x, scores, look_every)

    def _dev_buffers(self, B, S, n, x, scores, look_every, exact=True):
        """... for batches of up to B rows (exact=False: the element counts are left to the library's own extent check)"""
        torch = N.torch_first()
        dts = {torch.float32: N.FB_DT_F32, torch.float64: N.FB_DT_F64}
        for name, t, want in (("x", x, B * n), ("scores", scores, B * S)):
            if not isinstance(t, torch.Tensor):
                raise TypeError("%s must be a torch tensor (got %s)" % (name, type(t).__name__))
            if t.device.type != "cuda" or t.device.index != self.device:
                raise ValueError("%s is on %s: the device path needs a tensor on cuda:%d" % (name, t.device, self.device))
            if t.dtype not in dts:
                raise ValueError("%s has dtype %s: float32 or float64" % (name, t.dtype))
            if not t.is_contiguous() or (exact and t.numel() != want):
                raise ValueError("%s must be contiguous with %d elements (got %s)" % (name, want, tuple(t.shape)))
        m = N.DevModel()
        m.x_dtype, m.x = dts[x.dtype], x.data_ptr()
        m.score_dtype, m.scores = dts[scores.dtype], scores.data_ptr()
        m.look_every = int(look_every)
        N.check_one_hip_runtime()
        return m

    def _score_dev_cb(self, score_fn, x, scores, S, err):
        """score_fn(x) -> [B, S] scores on the device, run on the engine's stream and copied into `scores`, wrapped as an
        fb_score_dev_cb.  x is the engine's batch buffer itself, rewritten by the next iteration.  An exception raised by
        the model is kept in err[0] and re-raised by the caller, as _score_cb does."""
        torch = N.torch_first()
        ext = []

        def _cb(_ctx, stream, n, b, s):
            try:
                if not ext:
                    ext.append(torch.cuda.ExternalStream(stream, device=torch.device("cuda", self.device)))
                with torch.cuda.stream(ext[0]):
                    # (the first b rows: a batch of the swarm and decision attacks may be smaller than the buffers)
                    out = score_fn(x.view(-1)[:b * n].view(b, n))
                    if not isinstance(out, torch.Tensor):
                        out = torch.as_tensor(out, device=scores.device)
                    scores.view(-1)[:b * s].view(b, s).copy_(out.reshape(b, s))
                return 0
            except BaseException as ex:  # noqa: BLE001
                err[0] = ex
                return 1
        return N.SCORE_DEV_CB(_cb)

    def _device_model(self, params, S, score_fn, x, scores, look_every):
        def model(n):
            m = self._dev_model(params, S, n, x, scores, look_every)
            err = [None]
            return (C.c_int(S), C.byref(m), self._score_dev_cb(score_fn, x, scores, S, err), None), err
        return model

    def get_grad_dev(self, params, S, score_fn, x, scores, audio, it=0, noise_pos=None):
        """fb_get_grad_dev: one NES gradient estimate at `audio`, the batch written into the torch tensor x [B, N] and
        scored by score_fn on the GPU into scores [B, S]."""
        return self._get_grad("fb_get_grad_dev", params, S, audio, it, noise_pos,
                              model=self._device_model(params, S, score_fn, x, scores, 0))

    def attack_dev(self, params, S, score_fn, x, scores, audio, noise_all=None, look_every=0):
        """fb_attack_dev: the whole attack loop around a model on the GPU -> (int16 adv, flag, float64 adv, trace).
        look_every: iterations between the host's looks at the loop control (0: 4)."""
        return self._attack("fb_attack_dev", params, S, audio, noise_all,
                            model=self._device_model(params, S, score_fn, x, scores, look_every))

    _FOREIGN_PATH = {1: "host", 2: "device"}
    _DT = {0: "float32", 1: "float64"}

    def debug_foreign_path(self):
        """The last foreign-model call (fb_debug_foreign_path): a dict of path ("host" / "device"), x_dtype and
        score_dtype, launches_per_iter, model_calls, batch_bytes_d2h and score_bytes_h2d (during the loop)."""
        info = N.ForeignPathInfo()
        N.check(self._L.fb_debug_foreign_path(self._h, C.byref(info)))
        return dict(path=self._FOREIGN_PATH[info.path], x_dtype=self._DT[info.x_dtype],
                    score_dtype=self._DT[info.score_dtype], launches_per_iter=int(info.launches_per_iter),
                    model_calls=int(info.model_calls), batch_bytes_d2h=int(info.batch_bytes_d2h),
                    score_bytes_h2d=int(info.score_bytes_h2d))

    _NES_ROUTE = ("iv_tail", "fin_loss", "fin_loss_update", "k_loss", "k_update_perturb", "k_grad_update")

    def debug_nes_route(self):
        """Where the loss and the momentum step of the last get_grad* / attack* call ran (fb_debug_nes_route): a dict of
        launch counts -- iv_tail, fin_loss, fin_loss_update, k_loss, k_update_perturb, k_grad_update -- one per NES
        iteration the call queued."""
        info = (C.c_int * len(self._NES_ROUTE))()
        N.check(self._L.fb_debug_nes_route(self._h, info))
        return dict(zip(self._NES_ROUTE, (int(v) for v in info)))

    def debug_nes_batch(self, n, half, want_q=True, want_z=True):
        """The NES batch the last get_grad* / attack* / bench_nes call left on the device (fb_debug_nes_batch; read only) ->
        (q, z, iter): q (2 half + 1, n) int16, the batch of the engine's own systems (None without want_q: a foreign
        model's batch is in its x), z (half, n) float32, the normals kept for the gradient (None without want_z: a call on
        injected normals keeps none), iter the Philox iteration index the rows were drawn for."""
        q = np.empty((2 * half + 1, n), np.int16) if want_q else None
        z = np.empty((half, n), np.float32) if want_z else None
        it = C.c_longlong()
        N.check(self._L.fb_debug_nes_batch(self._h, C.c_int64(n), C.c_int(half), None if q is None else N.ptr(q),
                                           None if z is None else N.ptr(z), C.byref(it)))
        return q, z, it.value

    def estimate_threshold(self, params, model_threshold, audio, noise_all=None, max_total_iters=100000):
        audio = np.ascontiguousarray(audio, np.float64).reshape(-1)
        n = audio.size
        na = None if noise_all is None else np.ascontiguousarray(noise_all, np.float64)
        sc, tf = C.c_double(), C.c_double()
        ni, no = C.c_int(), C.c_int()
        adv_f = np.empty(n, np.float64)
        N.check(self._L.fb_estimate_threshold(self._h, C.byref(params), C.c_double(model_threshold),
                                              N.ptr(audio), C.c_int64(n), None if na is None else N.ptr(na),
                                              C.c_int(max_total_iters), C.byref(sc), C.byref(ni), C.byref(no),
                                              C.byref(tf), N.ptr(adv_f)))
        return sc.value, ni.value, no.value, tf.value, adv_f

    # ---- debug / bench hooks
    def debug_noise(self, seed, it, stream, n, half):
        z = np.empty((half, n), np.float32)
        N.check(self._L.fb_debug_noise(self._h, C.c_uint64(seed), C.c_uint32(it), C.c_uint32(stream),
                                       C.c_int64(n), C.c_int(half), N.ptr(z)))
        return z

    def debug_quantize(self, x, bits_per_sample=16):
        x = np.ascontiguousarray(x, np.float64).reshape(-1)
        q = np.empty(x.size, np.int16)
        N.check(self._L.fb_debug_quantize(self._h, N.ptr(x), C.c_int64(x.size), C.c_int(bits_per_sample), N.ptr(q)))
        return q

    def _num_frames(self, n):
        c = self.cfg
        if c.snip_edges:
            return 0 if n < c.frame_length else 1 + (n - c.frame_length) // c.frame_shift
        return (n + c.frame_shift // 2) // c.frame_shift

    def debug_mfcc(self, wav):
        wav = np.ascontiguousarray(wav, np.int16)
        T = self._num_frames(wav.size)
        out = np.empty((T, self.cfg.num_ceps), np.float32)
        To = C.c_int()
        N.check(self._L.fb_debug_mfcc(self._h, N.ptr(wav), C.c_int64(wav.size), N.ptr(out), C.byref(To)))
        return out[:To.value]

    def debug_feats(self, wav):
        wav = np.ascontiguousarray(wav, np.int16)
        T = self._num_frames(wav.size)
        out = np.empty((max(T, 1), self.feat_dim), np.float32)
        tv, To = C.c_int(), C.c_int()
        N.check(self._L.fb_debug_feats(self._h, N.ptr(wav), C.c_int64(wav.size), N.ptr(out), C.byref(tv),
                                       C.byref(To)))
        return out[:tv.value].copy(), To.value

    def debug_dither_noise(self, seed, stream, epoch, utt, t0, n_frames, L=None):
        """The normals (n_frames, L) the dithered MFCC kernels add to frames t0 .. of utterance `utt` at (seed, stream,
        epoch) -- fb_debug_dither_noise."""
        L = self.cfg.frame_length if L is None else int(L)
        z = np.empty((int(n_frames), L), np.float32)
        N.check(self._L.fb_debug_dither_noise(self._h, C.c_uint64(int(seed)), C.c_uint32(int(stream)), C.c_uint32(int(epoch)),
                                              C.c_uint32(int(utt)), C.c_int(int(t0)), C.c_int(int(n_frames)), C.c_int(L),
                                              N.ptr(z)))
        return z

    def debug_mfcc_dither(self, wav, seed, stream, epoch, utt):
        """debug_mfcc of one utterance at that point of the dither contract (fb_debug_mfcc_dither)."""
        wav = np.ascontiguousarray(wav, np.int16)
        T = self._num_frames(wav.size)
        out = np.empty((T, self.cfg.num_ceps), np.float32)
        To = C.c_int()
        N.check(self._L.fb_debug_mfcc_dither(self._h, N.ptr(wav), C.c_int64(wav.size), C.c_uint64(int(seed)),
                                             C.c_uint32(int(stream)), C.c_uint32(int(epoch)), C.c_uint32(int(utt)),
                                             N.ptr(out), C.byref(To)))
        return out[:To.value]

    def debug_feats_dither(self, wav, seed, stream, epoch, utt):
        """debug_feats of one utterance at that point of the dither contract (fb_debug_feats_dither)."""
        wav = np.ascontiguousarray(wav, np.int16)
        T = self._num_frames(wav.size)
        out = np.empty((max(T, 1), self.feat_dim), np.float32)
        tv, To = C.c_int(), C.c_int()
        N.check(self._L.fb_debug_feats_dither(self._h, N.ptr(wav), C.c_int64(wav.size), C.c_uint64(int(seed)),
                                              C.c_uint32(int(stream)), C.c_uint32(int(epoch)), C.c_uint32(int(utt)),
                                              N.ptr(out), C.byref(tv), C.byref(To)))
        return out[:tv.value].copy(), To.value

    def debug_gmm_frames(self, feats):
        """Per-frame log-likelihoods [M, T] of `feats` [T, D] from the GMM kernel the engine scores with (test hook)."""
        feats = np.ascontiguousarray(feats, np.float32)
        T = feats.shape[0]
        out = np.empty((self.n_models, T), np.float64)
        N.check(self._L.fb_debug_gmm_frames(self._h, N.ptr(feats), C.c_int(T), N.ptr(out)))
        return out

    def debug_gmm_acc_rows(self, feats, want_ll=False):
        """Enrolment statistics of `feats` [T, D] handed in as they are: the launches of gmm_acc_stats without its
        front-end (test hook).  -> occ[C], F[C, D] (float64), and with want_ll the dump matrix ll[T, C] (float32)."""
        feats = np.ascontiguousarray(feats, np.float32)
        Cn, D = self._gmm_shape
        if feats.ndim != 2 or feats.shape[1] != D:
            raise ValueError("debug_gmm_acc_rows takes rows of %d features" % D)
        T = feats.shape[0]
        occ = np.empty(Cn, np.float64)
        F = np.empty((Cn, D), np.float64)
        ll = np.empty((T, Cn), np.float32) if want_ll else None
        N.check(self._L.fb_debug_gmm_acc_rows(self._h, N.ptr(feats), C.c_int(T), N.ptr(ll) if want_ll else None,
                                              N.ptr(occ), N.ptr(F)))
        return (occ, F, ll) if want_ll else (occ, F)

    def stats(self):
        a, b, c, d = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64()
        N.check(self._L.fb_stats(self._h, C.byref(a), C.byref(b), C.byref(c), C.byref(d)))
        return dict(scored_utts=a.value, scored_frames=b.value, voiced_frames=c.value, nes_iters=d.value)

    def bench_gmm_kernel(self, reps=20):
        ms, rows = C.c_double(), C.c_int64()
        N.check(self._L.fb_bench_gmm_kernel(self._h, C.c_int(reps), C.byref(ms), C.byref(rows)))
        return ms.value, rows.value

    def set_fused_chain(self, on):
        """True: 4 launches per NES iteration (best for one or two attacks per GPU); False: 6 launches, finalisation and loss on their own (better
        with >= 3 engines sharing a GPU -- and once three engines on the device are set to it, no drain between looks:
        debug_shared_chain_engines); None: library default.  Same trajectories (fb_set_fused_chain)."""
        N.check(self._L.fb_set_fused_chain(self._h, C.c_int(-1 if on is None else (1 if on else 0))))

    def debug_shared_chain_engines(self):
        """Engines of this process on this engine's device with set_fused_chain(False) (fb_debug_shared_chain_engines)."""
        n = C.c_int()
        N.check(self._L.fb_debug_shared_chain_engines(self._h, C.byref(n)))
        return n.value

    def bench_nes(self, params, audio, warmup, iters, time_gmm=False):
        """Runs warmup+iters NES iterations (identical work to attack(), early stop disabled).
        Returns (ms over the timed iters [HIP events], summed GMM-kernel ms [HIP events around
        each launch on the engine stream], voiced rows of the last batch)."""
        audio = np.ascontiguousarray(audio, np.float64).reshape(-1)
        ms, msg, rows = C.c_double(), C.c_double(), C.c_int64()
        N.check(self._L.fb_bench_nes(self._h, C.byref(params), N.ptr(audio), C.c_int64(audio.size),
                                     C.c_int(warmup), C.c_int(iters), C.c_int(int(time_gmm)),
                                     C.byref(ms), C.byref(msg), C.byref(rows)))
        return ms.value, msg.value, rows.value

    def bench_nes_state(self, params, n):
        """What the attack bench_nes left on the device holds after its last iteration (fb_bench_nes_state): a dict of
        adver (n,) the adversarial audio, scores (B, S) and loss (B,) of the last NES batch (row 0 = the unperturbed
        adversarial audio), final_loss, adver_loss, distance.  `params` / `n`: those of the bench_nes calls."""
        B = 2 * (params.samples_per_draw // 2) + 1
        adver = np.empty(int(n), np.float64)
        scores = np.empty((B, max(self.n_speakers, 1)), np.float64)
        loss = np.empty(B, np.float64)
        summary = np.empty(3, np.float64)
        N.check(self._L.fb_bench_nes_state(self._h, N.ptr(adver), N.ptr(scores), N.ptr(loss), N.ptr(summary)))
        return dict(adver=adver, scores=scores, loss=loss, final_loss=summary[0], adver_loss=summary[1], distance=summary[2])
