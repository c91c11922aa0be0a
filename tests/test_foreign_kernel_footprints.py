"""The two kernels between the query attacks' int16 batch and a foreign victim (csrc/foreign_rows_kernel.hip) use no scratch
memory: k_rows_to_model is a pure bandwidth pass and k_decide_foreign a row scan, neither has anything to spill.  The method
is tests/test_kernel_footprints.py's: the source compiled device-only with the flags of fakebob_amd.build and
-Rpass-analysis=kernel-resource-usage, the compiler's own figures read; no instruction is looked at."""
from tests.test_kernel_footprints import _usage

# every instantiation, by the start of its mangled name: k_rows_to_model<float | double, vector | element-wise>,
# k_decide_foreign<float | double>
KERNELS = ("_Z15k_rows_to_modelIfLb1EE", "_Z15k_rows_to_modelIfLb0EE", "_Z15k_rows_to_modelIdLb1EE", "_Z15k_rows_to_modelIdLb0EE",
           "_Z16k_decide_foreignIfE", "_Z16k_decide_foreignIdE")


def test_the_foreign_victim_kernels_use_no_scratch(tmp_path):
    usage = _usage("foreign_rows_kernel.hip", str(tmp_path))
    for prefix in KERNELS:
        hits = [k for k in usage if k.startswith(prefix)]
        assert len(hits) == 1, (prefix, sorted(usage))
        u = usage[hits[0]]
        print("%s: %d VGPRs, %d bytes of scratch per lane" % (hits[0], u["VGPRs"], u["ScratchSize"]))
        assert u["ScratchSize"] == 0, (hits[0], u)
    assert len(usage) == len(KERNELS), sorted(usage)
