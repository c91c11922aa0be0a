"""What a component tile of k_gmm_fx2w may issue around its parameter fetches, and what the kernel may occupy.

One wave per SIMD issues in order, and a P = 1 tile is short of issue slots, so an instruction that does no
arithmetic costs what any other does.  Two kinds used to sit in the tile: three s_mov_b32 (a save, a set and a restore of M0), a
64-bit address add and an s_nop for every 1 KB global_load_lds_dwordx4, and 16 v_mov_b64 at the loop's back edge that copied an
accumulator set behind the tile's last MFMAs.  The pieces now go out in runs of up to four behind one M0 value and one address
(fb_glds16_at), and the copy is gone (the tile lambda of k_gmm_fx2w).

The test compiles gmm_wide_kernel.hip device-only with the flags of fakebob_amd.build, finds the P = 1 tile of
k_gmm_fx2w<5, 6> in the compiler's own output -- the innermost loop that holds exactly the tile's 110 MFMAs -- and counts by
opcode family: v_mfma, global_load_lds_dwordx4, v_mov_b64, s_mov_b32, s_nop.  Nothing else is looked for.  The kernels'
footprints come from the same output's metadata and must not exceed those of the build before the fetch runs."""
import os
import re
import subprocess

import pytest

from fakebob_amd import build as B

KERNEL = "_Z10k_gmm_fx2wILi5ELi6EE"
TILE_MFMAS = 30 + 30 + 5 * 10      # Q, base model, five delta items of one product per K chunk
TILE_PIECES = 18                   # per wave: group B (3 items x 10 KB / 4 waves -> 8) + group A of the next tile (4 items -> 10)
# 5 pieces go out at the head of a group and 5 per step after it: 5 (4 + 1) and 3 for group B, 5 (4 + 1) and 5 (4 + 1) for A
TILE_RUNS = 7
# (vector + accumulation registers, SGPR spills) of k_gmm_fx2w<5, M> before this change; scratch was and stays 0
BEFORE = {2: (352, 27), 3: (392, 34), 4: (397, 43), 5: (412, 48), 6: (420, 56), 7: (426, 58), 8: (438, 66), 9: (447, 79),
          10: (453, 87)}


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    src = "gmm_wide_kernel.hip"
    out = str(tmp_path_factory.mktemp("fxw_asm") / "gmm_wide_kernel.s")
    cmd = ([B._hipcc()] + B.FLAGS + B.SOURCE_FLAGS.get(src, []) +
           ["--cuda-device-only", "-S", os.path.join(B.CSRC, src), "-o", out])
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-4000:]
    with open(out) as f:
        return f.read()


def _function(text, prefix):
    """the instructions and block labels of the function whose mangled name starts with prefix, in layout order"""
    lines = text.splitlines()
    start = next(i for i, l in enumerate(lines) if l.startswith(prefix) and l.split(";")[0].rstrip().endswith(":"))
    end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
    out = []
    for l in lines[start + 1:end]:
        t = l.split(";")[0].strip()
        m = re.match(r"^(\.LBB\d+_\d+):$", t)
        if m:
            out.append(("label", m.group(1)))
        elif t and not t.startswith("."):
            out.append(("ins", t))
    return out


def _tile(fn):
    """the innermost loop (block label .. backward branch to it) with exactly the tile's MFMAs and fetches"""
    pos = {name: i for i, (kind, name) in enumerate(fn) if kind == "label"}
    best = None
    for i, (kind, t) in enumerate(fn):
        if kind == "ins" and t.startswith(("s_branch", "s_cbranch")):
            target = t.split()[-1]
            if target in pos and pos[target] < i:
                body = [x for k, x in fn[pos[target]:i + 1] if k == "ins"]
                if (sum(x.startswith("v_mfma") for x in body) == TILE_MFMAS and
                        sum(x.startswith("global_load_lds_dwordx4") for x in body) == TILE_PIECES):
                    if best is None or len(body) < len(best):
                        best = body
    return best


def _around_fetches(body, family):
    """instructions of `family` in the unbroken runs of s_mov_b32 / s_nop directly in front of and behind each fetch"""
    n = 0
    for i, x in enumerate(body):
        if x.startswith("global_load_lds_dwordx4"):
            for step in (-1, 1):
                j = i + step
                while 0 <= j < len(body) and body[j].startswith(("s_mov_b32", "s_nop")):
                    n += body[j].startswith(family)
                    j += step
    return n


def test_p1_tile_of_the_benchmark_kernel_has_no_copies_and_one_set_up_per_run(asm):
    body = _tile(_function(asm, KERNEL))
    assert body is not None, "no loop with %d MFMAs and %d fetches in %s" % (TILE_MFMAS, TILE_PIECES, KERNEL)
    count = {f: sum(x.startswith(f) for x in body) for f in ("v_mfma", "global_load_lds_dwordx4", "v_mov_b64", "s_mov_b32", "s_nop")}
    print("P = 1 tile of k_gmm_fx2w<5, 6>: %d instructions, %s; around the fetches: %d s_mov_b32, %d s_nop" %
          (len(body), count, _around_fetches(body, "s_mov_b32"), _around_fetches(body, "s_nop")))
    assert count["v_mov_b64"] == 0, "an accumulator set is copied inside the tile again"
    # at most two s_mov_b32 and two s_nop per run of up to four pieces -- in the whole tile, whatever they are for
    assert count["s_mov_b32"] <= 2 * TILE_RUNS, count
    assert _around_fetches(body, "s_nop") <= 2 * TILE_RUNS
    # every piece but a run's first takes its place from the instruction's offset
    with_offset = sum(x.startswith("global_load_lds_dwordx4") and "offset:" in x for x in body)
    assert with_offset == TILE_PIECES - TILE_RUNS, (with_offset, [x for x in body if x.startswith("global_load_lds_dwordx4")])


def test_wide_kernel_footprints_did_not_grow(asm):
    meta = asm[asm.index("amdhsa.kernels:"):]
    seen = {}
    for blk in meta.split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        m = re.match(r"_Z10k_gmm_fx2wILi5ELi(\d+)EE", name)
        if not m:
            continue
        get = lambda key: int(re.search(r"\.%s:\s+(\d+)" % key, blk).group(1))  # noqa: E731
        regs, spills = get("vgpr_count"), get("sgpr_spill_count")   # (vgpr_count: vector + accumulation registers)
        seen[int(m.group(1))] = (regs, spills)
        assert get("private_segment_fixed_size") == 0 and get("vgpr_spill_count") == 0, name
        assert get("group_segment_fixed_size") == 0, name           # (the kernel's LDS is all dynamic: fb_launch_gmm_wide)
    print("k_gmm_fx2w<5, M>: (registers, SGPR spills) %s" % seen)
    assert sorted(seen) == sorted(BEFORE)
    for m_, (regs, spills) in seen.items():
        assert regs <= BEFORE[m_][0] and spills <= BEFORE[m_][1], (m_, regs, spills, BEFORE[m_])
