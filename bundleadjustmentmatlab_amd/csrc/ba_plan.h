// ba_plan.h -- the context's host planner: the observation sort, the
// co-visible block set, the point order by track kind and the chunk / group
// plan of the fast Schur path (ba_plan.cpp).  Host only: no HIP, RCCL or
// rocSOLVER header, so the planner builds with any C++17 compiler
// (tools/bench_plan.cpp hashes its plans, tests/test_plan_sanitize.py runs it
// under the sanitizers).  ba_solver.cpp's ctx_create / ctx_setup (and the
// setup_* pieces of the latter) call it and upload what it returns.
#pragma once
#include "ba_limits.h"
#include "../../include/vlgba.h"

#include <stddef.h>
#include <utility>
#include <vector>

// internal to libvlgba.so: not part of its exported ABI
#pragma GCC visibility push(hidden)

// Observation list sorted point-major: points ascending, cameras ascending
// within a point (the order of the reference's column-major n x m loops).
struct host_obs {
    std::vector<int> pt, cam;
    std::vector<double> x;
};
int sort_obs(const vlgba_problem *p, host_obs &h);

// Co-visible camera-pair blocks and their term lists (obs pairs, point
// ascending).  lower: blocks j >= k only (the Cholesky reads the lower
// triangle); otherwise all ordered pairs (stage-2 entry: full S like
// mex_bundle_2_Se_.c).  The block SET comes from all observations (so every
// rank agrees on the packed layout); terms only from observations [o0, o1).
struct host_blocks {
    std::vector<int> jk, ptr, term;
    int m = 0;
    bool dense_tab = true;
    std::vector<int> tab;                                // m*m block ids (dense)
    std::vector<std::vector<std::pair<int, int>>> rows;  // sparse fallback: (k, id)
    // empty, keeping the vectors' capacity (a context per growing-replay solve:
    // reused storage is not page-faulted in again, ctx_setup's per-thread pool)
    // The dense table stays allocated and all -1 between contexts: reset()
    // clears the entries this context's blocks set (O(blocks) instead of
    // rewriting m x m ints -- 3.2 MB at 900 cameras -- per context).
    void reset()
    {
        if (dense_tab && !tab.empty())
            for (size_t q = 0; q + 1 < jk.size(); q += 2) tab[(size_t)jk[q] * m + jk[q + 1]] = -1;
        jk.clear();
        ptr.clear();
        term.clear();
        m = 0;
        dense_tab = true;
        rows.clear();
    }
    int find(int j, int k) const
    {
        if (dense_tab) return tab[(size_t)j * m + k];
        for (auto &pr : rows[j])
            if (pr.first == k) return pr.second;
        return -1;
    }
    int insert(int j, int k)
    {
        int id = find(j, k);
        if (id >= 0) return id;
        id = (int)jk.size() / 2;
        jk.push_back(j);
        jk.push_back(k);
        if (dense_tab) tab[(size_t)j * m + k] = id;
        else rows[j].push_back({k, id});
        return id;
    }
};
void build_blocks(int m, const std::vector<int> &pt_ptr_all, const std::vector<int> &cam_all,
                  int p0, int p1, long long obs_base, bool lower, bool all_diag, bool need_terms,
                  host_blocks &hb);

// Chunk plan of the fast Schur path for the local points (pt_ptr local,
// cam local observation cameras).  Points [0, p_split) form MFMA chunks
// (k_schur_mfma), points [p_split, n) per-term chunks (k_schur_group); the
// chunk and group sequences keep that order, so the MFMA groups are
// [0, ngrp_mf) and the term groups [ngrp_mf, ngrp).  Returns false when a
// point does not fit its chunk kind (the caller then uses the ordered kernels).
struct host_plan {
    std::vector<int> ch_pt, ch_slot, ch_eslot, slot_blk, slot_tptr, eslot_optr;
    std::vector<unsigned short> slot_term, eslot_obs;
    std::vector<int> cam_eptr, cam_eslots;
    int max_terms = 0, max_slots = 0;   // per chunk (LDS staging size)
    long long n_terms = 0;              // (obs, obs) Schur terms of all chunks
    // Schur groups: consecutive chunks whose co-visible blocks ("group slots")
    // and cameras ("group e-slots") are accumulated in LDS across the group
    std::vector<int> grp_ch, grp_gs, grp_ge;      // [ngrp+1] ranges
    std::vector<unsigned short> cs_g, ce_g;        // chunk slot / e-slot -> group-local id
    std::vector<int> gslot_blk, gecam;             // [ngs], [nge]
    std::vector<int> blk_gptr, blk_gslots, cam_gptr, cam_gslots;
    int grp_max_s = 0, grp_max_e = 0;             // largest accumulated term group
    int mf_max_s = 0, mf_max_e = 0;               // largest MFMA group
    int nch_mf = 0, ngrp_mf = 0;                  // leading MFMA chunks / groups
    // long tracks (points [p_long, n)): each split into segment chunks of <=
    // BA_CH_OBS observations (after the regular chunks: chunk ids
    // [nch_reg, nch_reg + nseg)); their Schur terms are group slots of their
    // own, one per (obs, obs) pair, and one group e-slot per observation
    int nch_reg = 0, nseg = 0;
    std::vector<int> seg_pt, seg_long;            // [nseg] point / long index
    std::vector<int> long_pt, long_o0, long_seg0; // [nl], [nl+1], [nl+1]
    std::vector<int> long_ebase;                  // [nl] first group e-slot
    std::vector<int> cam_lptr, cam_lobs, cam_ltrk; // per camera its long observations
    int max_lcam = 0;                             // (long-obs index, track), track order
    // per chunk one contiguous metadata record (one coalesced prefetch):
    //   [np | nobs << 16][ns | nes << 16][nterm][neobs] soff[ns+1] eoff[nes+1]
    //   sgl[ns] egl[nes] lpt[nobs] term[nterm] (y | w << 16) eobl[neobs]
    std::vector<unsigned> blob;
    std::vector<int> ch_blob, ch_obase;            // [nch+1]
    int max_blob = 0;      // term chunks: largest record
    int mf_max_blob = 0;   // MFMA groups: largest group record block (staged in LDS)
    // empty, keeping every vector's capacity (host_blocks::reset)
    void reset()
    {
        for (std::vector<int> *v :
             {&ch_pt, &ch_slot, &ch_eslot, &slot_blk, &slot_tptr, &eslot_optr,
              &cam_eptr, &cam_eslots, &grp_ch, &grp_gs, &grp_ge, &gslot_blk, &gecam,
              &blk_gptr, &blk_gslots, &cam_gptr, &cam_gslots, &seg_pt, &seg_long, &long_pt,
              &long_o0, &long_seg0, &long_ebase, &cam_lptr, &cam_lobs, &cam_ltrk, &ch_blob,
              &ch_obase})
            v->clear();
        for (std::vector<unsigned short> *v : {&slot_term, &eslot_obs, &cs_g, &ce_g}) v->clear();
        blob.clear();
        max_terms = max_slots = 0;
        n_terms = 0;
        grp_max_s = grp_max_e = mf_max_s = mf_max_e = nch_mf = ngrp_mf = 0;
        nch_reg = nseg = max_lcam = max_blob = mf_max_blob = 0;
    }
};
// 0: MFMA Schur chunk (<= cmax views), 1: per-term chunk, 2: long track
int track_kind(long long k, int cmax);
void order_points_by_kind(int cmax, host_obs &h, std::vector<int> &pt_ptr, int p0, int p1,
                          std::vector<int> &pperm, std::vector<int> &operm);
// mark("blocks") is called once the block set stands (ctx_setup's setup trace)
void plan_host(int m, int na, int n, const std::vector<int> &lptr, const std::vector<int> &lcam,
               const std::vector<int> &pt_ptr_all, const std::vector<int> &cam_all, int p0,
               int p1, long long o0, bool lower_blocks, bool all_diag, bool no_mfma, bool &fast,
               int &p_long, host_blocks &hb, host_plan &plan,
               void (*mark)(const char *) = nullptr);

// What ctx_setup derives from a fast plan before it uploads it.
// The MFMA groups are the only Schur groups and tile the points [0, n)
// (V*^-1 inside k_schur_mfma, ba_dev::vinv_fold):
bool plan_mfma_groups_tile_points(const host_plan &plan, int n);
// chunk-local point of every observation (k_linearize_chunk), at least one entry:
void plan_obs_local_point(const host_plan &plan, const std::vector<int> &lptr,
                          std::vector<unsigned char> &lpt);
// each chunk's lowest / highest camera (k_update_linearize's da staging), at
// least one pair:
void plan_chunk_cameras(const host_plan &plan, const std::vector<int> &lcam,
                        std::vector<int> &ccam);

#pragma GCC visibility pop
