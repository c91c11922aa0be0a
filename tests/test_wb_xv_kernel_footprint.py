"""The kernels of csrc/whitebox_xv_kernels.hip -- the TDNN's backward -- keep their working set in registers and static LDS:
no scratch memory in any of them, and at most 64 KB of LDS per workgroup.  The compiler's own figures, by the recipe of
tests/test_xvector_kernel_footprint.py."""
import os
import re
import subprocess

from fakebob_amd import build as B

SRC = "whitebox_xv_kernels.hip"
KERNELS = ("k_wb_xv_segment_t", "k_wb_xv_pool_t", "k_wb_xv_act_t", "k_wb_xv_affine_t", "k_wb_xv_unsplice")


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


def test_the_file_is_built_into_the_library():
    assert SRC in B.SOURCES and os.path.exists(os.path.join(B.CSRC, SRC))


def test_no_kernel_of_the_tdnn_backward_uses_scratch(tmp_path):
    usage = _usage(str(tmp_path))
    for kernel in KERNELS:                      # one plain kernel each: no template instantiations
        names = [k for k in usage if re.match(r"_Z\d+%s[A-Z0-9]" % kernel, k)]
        assert len(names) == 1, (kernel, sorted(usage))
    assert len(usage) == len(KERNELS), sorted(usage)
    for k, u in sorted(usage.items()):
        print("%s: VGPRs %d AGPRs %d scratch %d LDS %d bytes, %d waves per SIMD" %
              (k, u["VGPRs"], u["AGPRs"], u["ScratchSize"], u["LDS"], u["Occupancy"]))
        assert u["ScratchSize"] == 0, (k, u)
        assert u["LDS"] <= 64 * 1024, (k, u)    # static LDS: what a workgroup gets without an opt-in
