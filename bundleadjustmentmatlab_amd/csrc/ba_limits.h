// ba_limits.h -- chunk / group / long-track limits of the fast Schur path and
// the tile heights / nested-dissection / cyclic-reduction limits of the reduced
// solve, shared by the kernels (through ba_internal.h) and the host planners
// (ba_plan.h, ba_chol_plan.h).  Macros only: no HIP header, so host-only code
// can include it.
#pragma once

// reduced solve (ba_chol.hip, ba_chol_plan.cpp): rows of a Cholesky tile and of
// a camera-aligned cyclic-reduction tile (padded to it in LDS)
#define BA_TILE 64
#define BA_TILE32 32
// nested dissection of the envelope: at most this many camera arcs
#ifndef BA_ND_MAX
#define BA_ND_MAX 8
#endif
// ... and at most this many separator tile pairs (their SYRK partials: 33 KB
// each) / host checks (pairs x arc tiles) in its setup, else the natural order
#define BA_ND_MAX_PAIRS 16384LL
#define BA_ND_MAX_SETUP (1LL << 26)
// the one-launch cyclic reduction (k_cr32_fused) holds at most this many levels
#define BA_CR_MAXLEV 30

#ifndef BA_CH_OBS
#define BA_CH_OBS 128      // observations per Schur chunk (LDS budget)
#endif
#define BA_CH_PTS 64       // points per Schur chunk
#define BA_CH_TERMS 4096   // (obs, obs) terms per chunk: a track of <= 90 observations
#define BA_GACC 4096       // max doubles of LDS block accumulators per Schur group
#define BA_GE_CAP 128      // cameras per Schur group
#define BA_GROUPS 2048     // target number of Schur groups (workgroups)
#define BA_MF_GROUPS 768   // MFMA Schur groups: one round of 3 workgroups x 256 CUs
#define BA_GROUP_CH 64     // max chunks per Schur group
// MFMA Schur path (k_schur_mfma): a chunk is 4 K-blocks of 5 points (one per
// wave), its cameras span NA * cameras <= 16 * BA_MF_RT slab columns
#define BA_MF_PTS 20
#define BA_MF_RT(na) ((na) == 6 ? 3 : 4)
#define BA_MF_CMAX(na) ((16 * BA_MF_RT(na)) / (na))
#define BA_MF_GACC 1536    // doubles of LDS block accumulators per MFMA Schur group
#define BA_MF_GE_CAP 24    // cameras per MFMA Schur group (LDS budget: 2 groups per CU)
// long tracks (more observations than a chunk holds): segment chunks of
// BA_CH_OBS observations; their Schur terms are added per block by
// k_schur_reduce (merge of the two cameras' long-observation lists).  Caps
// (else the ordered kernels): views per track and (obs, obs) terms of all
// long tracks (the reduce's work)
#define BA_LONG_OBS 65535
#define BA_LONG_TERMS (1LL << 26)
// k_schur_reduce stages a camera's long-observation list in LDS up to this length
#define BA_LCAM_LDS 256
#define BA_LMATCH_BATCH 48   // ... and the matched Y / W rows this many terms at a time
