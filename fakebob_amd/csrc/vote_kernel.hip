// vote_kernel.hip -- k_vote: the voted decision of a candidate row that was scored r' times (fb_set_query_eot; the "voted
// decisions" section of include/fakebob_hip.h).  fb_attack_kenansville and fb_attack_hsj launch it behind the replicated
// scoring path in place of k_loss; the host reads its look block and nothing per replica.
//
// One wave64 per candidate row, four rows per workgroup.  Lane j < r' forms replica j's system scores with fb_loss_row -- the
// device function k_loss and k_loss_eot use, so the three cannot drift --, decides by the make_decisions rule and raises its
// flag; two ballots count the adversarial replicas and the replicas without a decision.  Then lane s < S adds the replicas'
// scores s in ascending rho and divides once: k_loss_eot's mean.  No atomics, no exchange between workgroups, no LDS; every
// sum has a fixed order, so a launch is reproducible bit for bit (tests/vote_ref.py restates it in numpy).
#include "fb_device.h"
#include "fb_kernels.h"
#include "fb_nes_device.h"

#define VOTE_BLOCK 256
#define VOTE_ROWS (VOTE_BLOCK / 64)

__global__ __launch_bounds__(VOTE_BLOCK) void k_vote(const double *__restrict__ raw, const int *__restrict__ tv, int rows, int r,
                                                     int M, int task, int znorm_all, const double *__restrict__ z_mean,
                                                     const double *__restrict__ z_std, double threshold, int targeted, int label,
                                                     double *__restrict__ rep_sc, int *__restrict__ votes,
                                                     int *__restrict__ nodec, double *__restrict__ mean) {
  const int S = (task == FB_TASK_CSI || znorm_all) ? M : M - 1;
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * VOTE_ROWS + (threadIdx.x >> 6);   // the wave's candidate row (uniform in the wave)
  const bool row_ok = b < rows;
  bool adv = false, none = false;
  if (row_ok && lane < r) {
    const int R = b * r + lane;   // (rows * r <= 65535)
    double *sc = rep_sc + (size_t)R * S;
    // (the loss is k_loss's untargeted one on label 0, as in the un-replicated attacks: formed and dropped)
    (void)fb_loss_row<false>(raw, R, M, S, task, znorm_all, FB_UNTARGETED, z_mean, z_std, threshold, 0.0, 0, 0, sc, nullptr);
    int d;
    if (tv[R] <= 0) {
      d = -2;   // no voiced frames: no decision, a failed replica
    } else if (task == FB_TASK_SV) {
      d = sc[0] >= threshold ? 1 : -1;
    } else {
      int am = 0;
      double best = sc[0];
      for (int m = 1; m < S; ++m) {   // the first maximum
        const double v = sc[m];
        if (v > best) { best = v; am = m; }
      }
      d = (task == FB_TASK_OSI && best < threshold) ? -1 : am;
    }
    none = d == -2;
    adv = !none && (targeted ? d == label : d != label);
  }
  // every lane of the wave takes part in the ballots; lanes >= r' and waves beyond the last row vote "no"
  const unsigned long long m_adv = __ballot(adv), m_none = __ballot(none);
  if (row_ok && lane == 0) {
    votes[b] = __popcll(m_adv);
    nodec[b] = __popcll(m_none);
  }
  __syncthreads();   // the replicas' score rows were written by other lanes of this workgroup
  if (row_ok) {
    const double *sr = rep_sc + (size_t)b * r * S;
    for (int s = lane; s < S; s += 64) {
      double a = sr[s];
      for (int j = 1; j < r; ++j) a = __dadd_rn(a, sr[(size_t)j * S + s]);
      mean[(size_t)b * S + s] = __ddiv_rn(a, (double)r);
    }
  }
}

void fb_launch_vote(hipStream_t s, const double *raw, const int *tv, int rows, int r, int M, int task, int znorm_all,
                    const double *z_mean, const double *z_std, double threshold, int targeted, int label, double *rep_sc,
                    int *votes, int *nodec, double *mean) {
  hipLaunchKernelGGL(k_vote, dim3((unsigned)((rows + VOTE_ROWS - 1) / VOTE_ROWS)), dim3(VOTE_BLOCK), 0, s, raw, tv, rows, r, M, task,
                     znorm_all, z_mean, z_std, threshold, targeted, label, rep_sc, votes, nodec, mean);
}
