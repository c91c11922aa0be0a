"""The gate of a tile-level skip in k_gmm_fx2w: CPU only, the oracle's front end and numpy.

The proposal: after a component tile's base item, test once per (tile, 32-frame half of a wave) whether the tile can still
matter to any frame's sum, and drop the tile's delta items -- 5 of its 11 MFMA items and 5/6 of its exponentials -- when it
cannot.  This script counts the (tile, half) pairs for which that would be SAFE, knowing everything: a pair counts when for
every frame of the half and every one of the six models the largest of the tile's 32 log-likelihoods lies more than
MARGIN_LOG2 binary orders below that model's running sum over the tiles of the same component chunk scored before it (the
kernel sums a chunk of 16 tiles per workgroup; the running sum starts empty with the chunk, so a chunk's first tile never
counts).  No test inside the kernel can skip more than this; the bar was 60 % of the pairs.

The batch is iteration 0 of the benchmark attack (bench.py's first attack: 3 s of synthetic audio, samples_per_draw = 50,
sigma = 0.001, Philox seed 42), its features the oracle's.  Rows: compact (an utterance's voiced frames in a row, as the
kernel has them) or frame-major (frame t of every utterance side by side, so that a half holds one frame under 32
perturbations).  Components: natural order, or tiles clustered by recursive bisection of the means along their principal
direction (2048 -> 64 groups of 32).

    python tools/probes/fxw_tile_skip_gate.py            # about a minute on 8 cores
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from fakebob_amd.models import synthetic_audio, synthetic_gmm_system  # noqa: E402
from oracle import oracle as O  # noqa: E402

TILE, HALF, CHUNKS = 32, 32, 4
MARGIN_LOG2 = 30.0
LOG2E = 1.0 / np.log(2.0)


def benchmark_batch(cfg, n=48000, spd=50, sigma=0.001, seed=42):
    """-> features (rows, D) float64 of the 51 utterances, compact; utterance and frame index of every row"""
    audio = synthetic_audio(0, n)
    half = spd // 2
    z = O.noise(seed, 0, 0, n, half).astype(np.float64)
    rows = [audio] + [audio + sigma * z[j] for j in range(half)] + [audio - sigma * z[j] for j in range(half)]
    feats, utt, frame = [], [], []
    for b, x in enumerate(rows):
        wav = O.quantize(np.clip(x, -1.0, 1.0))
        f, _ = O.frontend(cfg, wav)
        voiced = np.flatnonzero(O.vad(cfg, O.mfcc(cfg, wav)))
        assert voiced.size == f.shape[0], (b, voiced.size, f.shape)
        feats.append(f.astype(np.float64))
        utt.append(np.full(f.shape[0], b))
        frame.append(voiced)
    return np.concatenate(feats), np.concatenate(utt), np.concatenate(frame)


def bisect(means, idx, size):
    """groups of `size` components by recursive median splits along the principal direction of their means"""
    if idx.size <= size:
        return [idx]
    m = means[idx] - means[idx].mean(axis=0)
    _, _, vt = np.linalg.svd(m, full_matrices=False)
    order = idx[np.argsort(m @ vt[0], kind="stable")]
    h = (idx.size // 2 + size - 1) // size * size
    return bisect(means, order[:h], size) + bisect(means, order[h:], size)


def skippable_share(models, x, comp_order):
    """share of (tile, half) pairs whose delta items no model's sum would miss; x: the rows in the order under test"""
    rows = x.shape[0] // HALF * HALF     # (whole halves only: the last wave's tail is padding in the kernel)
    x = x[:rows]
    n_tiles = comp_order.size // TILE
    per_chunk = n_tiles // CHUNKS
    ok = np.ones((n_tiles, rows // HALF), bool)
    for m in models:
        g = m.gconsts.astype(np.float64)[comp_order]
        a = m.means_invvars.astype(np.float64)[comp_order]
        v = m.inv_vars.astype(np.float64)[comp_order]
        for c in range(CHUNKS):
            run = None   # log2 of the running sum of the chunk, per row
            for t in range(c * per_chunk, (c + 1) * per_chunk):
                k = slice(t * TILE, (t + 1) * TILE)
                ll = (g[k][None, :] + x @ a[k].T - 0.5 * (x * x) @ v[k].T) * LOG2E     # (rows, 32), log2 domain
                mx = ll.max(axis=1)
                if run is None:
                    ok[t] = False
                    run = mx + np.log2(np.exp2(ll - mx[:, None]).sum(axis=1))
                else:
                    ok[t] &= (mx < run - MARGIN_LOG2).reshape(-1, HALF).all(axis=1)
                    top = np.maximum(run, mx)
                    run = top + np.log2(np.exp2(run - top) + np.exp2(ll - top[:, None]).sum(axis=1))
    return ok.mean()


def main():
    cfg = O.default_cfg()
    ubm, spk = synthetic_gmm_system()
    models = [ubm] + spk
    x, utt, frame = benchmark_batch(cfg)
    print("%d voiced rows of %d utterances, %d models of %d components" % (x.shape[0], utt.max() + 1, len(models), ubm.gconsts.size))
    natural = np.arange(ubm.gconsts.size)
    means = ubm.means_invvars.astype(np.float64) / ubm.inv_vars.astype(np.float64)
    clustered = np.concatenate(bisect(means, natural, TILE))
    assert np.array_equal(np.sort(clustered), natural)
    frame_major = np.lexsort((utt, frame))
    print("%-46s %14s %18s" % ("component order", "compact rows", "frame-major rows"))
    for name, order in (("natural", natural), ("tiles clustered by bisection of the means", clustered)):
        print("%-46s %13.1f%% %17.1f%%" % (name, 100.0 * skippable_share(models, x, order),
                                            100.0 * skippable_share(models, x[frame_major], order)))


if __name__ == "__main__":
    main()
