"""What the small kernels of the shared-GPU launch chain may cost, so that they fit beside a resident k_gmm_fx2w workgroup.

With three or more attacks per GPU two half-chip k_gmm_fx2w launches of other attacks hold 240 of the 256 compute units most
of the time, one workgroup (four waves, one per SIMD) on each.  A SIMD has 512 registers; what the GMM wave leaves is all a
small kernel's waves can take there, and a kernel that needs more queues for the 16 units left over.
The test compiles the kernels' sources device-only with the flags of fakebob_amd.build and
-Rpass-analysis=kernel-resource-usage and reads the compiler's own figures: registers and scratch bytes, no instruction."""
import concurrent.futures as cf
import os
import re
import subprocess

from fakebob_amd import build as B

SOURCES = ("gmm_wide_kernel.hip", "nes_kernels.hip", "gmm_kernels.hip", "frontend_kernels.hip")
SIMD_REGS = 512   # a SIMD's unified register file (vector + accumulation), allocated in blocks of 8 per wave
# the kernels by the start of their mangled names: (waves per SIMD of one workgroup = threads / 256, must fit beside the GMM)
GMM = "_Z10k_gmm_fx2wILi5ELi6EE"
BESIDE = {
    "_Z16k_update_perturbILb1ELi256EE": 1,      # k_update_perturb<true, 256>: the shared chain's shape, 256 threads
    "_Z18k_vad_delta_cmvn_pILi2ELi3ELi24EE": 1,  # k_vad_delta_cmvn_p<2, 3, 24>: 256 threads
    "_Z14k_gmm_finalize": 1,                     # k_gmm_finalize: 256 threads
}
NO_SCRATCH = ("_Z16k_update_perturbILb1E", "_Z18k_update_perturb_xILb1E", "_Z6k_lossILb1E")


def _up8(n):
    return (n + 7) // 8 * 8


def _usage(src, tmp):
    cmd = ([B._hipcc()] + B.FLAGS + B.SOURCE_FLAGS.get(src, []) +
           ["--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(B.CSRC, src),
            "-o", os.path.join(tmp, src + ".o")])
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-4000:]
    out, cur = {}, None
    for m in re.finditer(r"remark:\s+([A-Za-z][^:\n]*): (\S+) \[-Rpass-analysis=kernel-resource-usage\]", r.stdout):
        key, val = m.group(1).strip(), m.group(2)
        if key == "Function Name":
            cur = out.setdefault(val, {})
        elif cur is not None and key in ("VGPRs", "AGPRs", "ScratchSize [bytes/lane]"):
            cur[key.split(" ")[0]] = int(val)
    return out


def test_small_kernels_fit_beside_a_gmm_workgroup(tmp_path):
    with cf.ThreadPoolExecutor(max_workers=len(SOURCES)) as ex:
        tables = list(ex.map(lambda s: _usage(s, str(tmp_path)), SOURCES))
    usage = {}
    for t in tables:
        usage.update(t)
    table = "\n".join("%-120s VGPRs %3d AGPRs %3d scratch %4d" % (k[:120], v.get("VGPRs", -1), v.get("AGPRs", -1),
                                                                   v.get("ScratchSize", -1)) for k, v in sorted(usage.items()))

    def find(prefix):
        hits = [k for k in usage if k.startswith(prefix)]
        assert hits, "no kernel named %s...\n%s" % (prefix, table)
        return hits

    (gmm,) = find(GMM)
    g = usage[gmm]
    leftover = SIMD_REGS - _up8(g["VGPRs"] + g["AGPRs"])
    assert 0 < leftover < SIMD_REGS, (g, table)
    print("k_gmm_fx2w<5, 6>: %d + %d registers, %d left per SIMD" % (g["VGPRs"], g["AGPRs"], leftover))
    for prefix, waves in BESIDE.items():
        (name,) = find(prefix)
        u = usage[name]
        need = waves * _up8(u["VGPRs"] + u["AGPRs"])
        print("%s: %d wave(s) x %d registers" % (prefix, waves, _up8(u["VGPRs"] + u["AGPRs"])))
        assert need <= leftover, "%s needs %d registers per SIMD, k_gmm_fx2w leaves %d\n%s" % (name, need, leftover, table)
    for prefix in NO_SCRATCH:
        for name in find(prefix):
            assert usage[name]["ScratchSize"] == 0, "%s uses scratch memory\n%s" % (name, table)
