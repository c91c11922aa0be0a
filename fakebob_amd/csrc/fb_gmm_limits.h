// fb_gmm_limits.h -- the numbers the GMM kernels (fb_kernels.h) and the host-side preparation of their images
// (fb_prepare.h) have to agree on.  No HIP here: both sides include it.
#pragma once
#define FB_FXW_MAX_PASS 3 // launches of k_gmm_fx2w per batch: 1 + 9 x 3 = 28 models (fb_gmm_delta_plan)
#define FB_FXW_MAX_M 10   // models ONE launch of k_gmm_fx2w takes: (1 + M) 10 KB items + the state of 2 M x 256 frames = 156 KB of LDS at M = 10
#define FB_FXW_ANCHORS 2  // anchor components of k_gmm_fx2w's per-frame reference (FbGmmDev::anchor)
#define FB_GMM_MODE_BX3 1
#define FB_GMM_MODE_FX2 2
