"""k_xv_affine (csrc/xvector_kernels.hip) keeps its four accumulator tiles and the fragments of a K step in registers: no
scratch memory.  The compiler's own figures, by the recipe of tests/test_kernel_footprints.py, with the LDS of a workgroup."""
import os
import re
import subprocess

from fakebob_amd import build as B

AFFINE = "_Z11k_xv_affine"
SRC = "xvector_kernels.hip"


def _usage(tmp):
    cmd = ([B._hipcc()] + B.FLAGS + B.SOURCE_FLAGS.get(SRC, []) +
           ["--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(B.CSRC, SRC), "-o", os.path.join(tmp, SRC + ".o")])
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-4000:]
    out, cur = {}, None
    for m in re.finditer(r"remark:\s+([A-Za-z][^:\n]*): (\S+) \[-Rpass-analysis=kernel-resource-usage\]", r.stdout):
        key, val = m.group(1).strip(), m.group(2)
        if key == "Function Name":
            cur = out.setdefault(val, {})
        elif cur is not None and key in ("VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "LDS Size [bytes/block]", "Occupancy [waves/SIMD]"):
            cur[key.split(" ")[0]] = int(val)
    return out


def test_k_xv_affine_uses_no_scratch(tmp_path):
    usage = _usage(str(tmp_path))
    (name,) = [k for k in usage if k.startswith(AFFINE)]
    u = usage[name]
    print("k_xv_affine: VGPRs %d AGPRs %d scratch %d LDS %d bytes, %d waves per SIMD" %
          (u["VGPRs"], u["AGPRs"], u["ScratchSize"], u["LDS"], u["Occupancy"]))
    assert u["ScratchSize"] == 0, "k_xv_affine uses scratch memory (%s)" % (u,)
    assert u["LDS"] <= 64 * 1024, u          # static LDS: what a workgroup gets without an opt-in
    for k, v in usage.items():               # nor does any other kernel of the file
        assert v["ScratchSize"] == 0, (k, v)
