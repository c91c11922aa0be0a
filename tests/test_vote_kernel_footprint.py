"""k_vote (fb_set_query_eot; csrc/vote_kernel.hip) beside a resident k_gmm_fx2w workgroup: the expectation of
tests/test_kernel_footprints.py for the launch that stands where k_loss stood in the decision-only attacks' replicated chain.
A workgroup of 256 threads is one wave per SIMD; it must fit into the registers the GMM wave leaves there, and it keeps its
replicas' scores in global memory (eot_sc), never in scratch memory.  The compiler's own figures, by that test's recipe."""
import concurrent.futures as cf

from tests.test_kernel_footprints import GMM, SIMD_REGS, _up8, _usage

VOTE = "_Z6k_vote"
SOURCES = ("gmm_wide_kernel.hip", "vote_kernel.hip")


def test_k_vote_fits_beside_a_gmm_workgroup(tmp_path):
    with cf.ThreadPoolExecutor(max_workers=len(SOURCES)) as ex:
        wide, vote = list(ex.map(lambda s: _usage(s, str(tmp_path)), SOURCES))
    (gmm,) = [k for k in wide if k.startswith(GMM)]
    (name,) = [k for k in vote if k.startswith(VOTE)]
    g, u = wide[gmm], vote[name]
    leftover = SIMD_REGS - _up8(g["VGPRs"] + g["AGPRs"])
    assert 0 < leftover < SIMD_REGS, g
    need = 1 * _up8(u["VGPRs"] + u["AGPRs"])            # 256 threads: one wave per SIMD
    print("k_gmm_fx2w<5, 6> leaves %d registers per SIMD; k_vote: 1 wave x %d registers, scratch %d" % (leftover, need, u["ScratchSize"]))
    assert need <= leftover, "k_vote needs %d registers per SIMD, k_gmm_fx2w leaves %d (%s)" % (need, leftover, u)
    assert u["ScratchSize"] == 0, "k_vote uses scratch memory (%s)" % (u,)
