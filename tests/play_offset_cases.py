"""The fixed cases of the composing launch under a play offset, shared by tests/test_gpu_play_offset.py (which runs them on
the device) and tests/test_play_offset_host.py (which shows on the restatement alone that they draw distinct offsets and a
wrap inside a workgroup's tile).  A case: (stage, n, S, K, eot) -- the defence in front of the victim, the samples per row,
the largest offset, the utterances per NES row and the draws per utterance.

Sizes: 257 (a row shorter than a tile, odd), 4000 and 4001 (a multiple of the 16-byte chunk and not: with 4001 most rows of
the flat batch start in the middle of a chunk and on an odd sample), 8200 (three chain tiles, five compose tiles).
Offsets: S = 1 (the wrap in a row's first chunk), 7 (inside one chunk), n - 1 (anywhere)."""
POINT = (11, 6, 3)          # seed, stream, epoch of the hook
ROWS = 5                    # NES rows of the hand-made batch
SIZES = (257, 4000, 4001, 8200)
AIR = "air64"               # an over-the-air channel of 64 taps in front of an empty chain

BIT_CASES = [("empty", n, S, 3, 4) for n in SIZES for S in (1, 7, n - 1)]
BIT_CASES += [("empty", n, n - 1, K, eot) for (K, eot) in ((1, 1), (1, 4), (3, 1)) for n in (257, 4001)]
ADPCM = "adpcm"             # the IMA ADPCM codec behind an empty chain: in place on the composed buffer
for _stage in ("ms:7,qt:512", "at:20", AIR, ADPCM):
    BIT_CASES += [(_stage, 4000, 7, 1, 4), (_stage, 4001, 4000, 3, 4), (_stage, 8200, 8199, 3, 1), (_stage, 257, 1, 1, 1)]
# ... and the codec behind a chain and behind the channel, where it runs in place on THEIR buffers ("stage|adpcm")
BIT_CASES += [("ms:7,qt:512|" + ADPCM, 4001, 4000, 3, 4), (AIR + "|" + ADPCM, 4001, 4000, 1, 4)]
