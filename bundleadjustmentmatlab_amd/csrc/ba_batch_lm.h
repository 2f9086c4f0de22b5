// ba_batch_lm.h -- host side of the batched one-block LM entries
// (vlgba_resect in ba_resect.hip: one camera, structure fixed; vlgba_intersect
// in ba_triang.hip: one point, motion fixed): the LM control of
// bundle_euclid.m:120-123, 205-241 applied per problem, each with its own
// lambda, and the per-device pool of a stream and a pinned staging block.
//
// Protocol of a pass.  stage() decides which problems go on (:120-123) and
// writes lambda and the flags word of every problem (as doubles, one copy a
// pass) into the pinned block; the pass kernel reads them with device-scope
// vector loads and writes four doubles per problem: old SSE, new SSE,
// dp'(lambda dp + g), pinv flag.  apply() reads those and applies :218-241.
// Under a loss (vlgba_resect_ex, vlgba_intersect_ex) the pass reports the robust
// cost and gradient in the same places; nothing here changes.
//   flags: 1 active | 2 linearise again (the parameters changed) | 4 the
//          previous pass was accepted (take x_new as x first)
#pragma once
#include "../../include/vlgba.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <vector>

// Per-device pool of a stream and a pinned host block for the per-pass LM
// scalars: creating a stream and pageable copies cost more than the
// resection itself (the growing-BA replay calls it once per added camera).
struct rs_pool {
    int device;
    hipStream_t s;
    double *pin;     // pinned: lam [np] | flags [np] (as doubles) | out [4 np]
    size_t cap;      // doubles
};
int rs_acquire(int device, size_t need, rs_pool &r);   // ba_resect.hip
void rs_release(const rs_pool &r);

// the mode arguments of the _ex entries: the kinds of vlgba_set_jacobian and
// vlgba_set_loss and the latter's scale rule; the radial model is analytic only
inline int batch_check_mode(int jacobian, int loss, double loss_scale, bool radial)
{
    if (jacobian != VLGBA_JAC_FD && jacobian != VLGBA_JAC_ANALYTIC) return VLGBA_E_ARG;
    if (radial && jacobian == VLGBA_JAC_FD) return VLGBA_E_ARG;
    if (loss < VLGBA_LOSS_NONE || loss > VLGBA_LOSS_CAUCHY) return VLGBA_E_ARG;
    if (loss != VLGBA_LOSS_NONE && !(std::isfinite(loss_scale) && loss_scale > 0))
        return VLGBA_E_ARG;
    return 0;
}

struct batch_lm {
    size_t np;
    int max_iter, max_iter2;
    double lambda0, stop_rel;
    std::vector<double> lam, nu;
    std::vector<int> fl, iter, iter2, passes, acc, active, accepted_prev, relin;
    std::vector<std::vector<double>> err;
    int total_passes = 0, total_acc = 0;

    // opt: max_iter, max_iter2, lambda0, stop_rel (0 -> the reference's)
    batch_lm(size_t np_, const vlgba_options *opt)
        : np(np_), max_iter(opt->max_iter > 0 ? opt->max_iter : 20),
          max_iter2(opt->max_iter2 > 0 ? opt->max_iter2 : 10),
          lambda0(opt->lambda0 > 0 ? opt->lambda0 : 1e-3),
          stop_rel(opt->stop_rel > 0 ? opt->stop_rel : 1e-3), lam(np_, lambda0), nu(np_, 2.0),
          fl(np_), iter(np_, 1), iter2(np_, 0), passes(np_, 0), acc(np_, 0), active(np_, 1),
          accepted_prev(np_, 0), relin(np_, 1), err(np_)
    {
    }

    // bundle_euclid.m:120-123 per problem; returns the number still active and
    // stages lambda / flags
    size_t stage(double *h_lam, double *h_fl)
    {
        size_t nact = 0;
        for (size_t q = 0; q < np; q++) {
            if (active[q]) {
                bool go = iter[q] < max_iter && iter2[q] < max_iter2;
                if (go && iter[q] >= 3) {
                    const double e1 = err[q][iter[q] - 1], e0 = err[q][iter[q] - 2];
                    go = e1 > 1e-20 && e0 - e1 > stop_rel * e0;
                }
                if (!go) active[q] = 0;
                nact += active[q];
            }
            fl[q] = active[q] | (relin[q] ? 2 : 0) | (accepted_prev[q] ? 4 : 0);
        }
        if (!nact) return 0;
        for (size_t q = 0; q < np; q++) {   // pinned staging: one small copy per pass
            h_lam[q] = lam[q];
            h_fl[q] = (double)fl[q];
        }
        return nact;
    }

    // bundle_euclid.m:218-241 per problem on the pass's scalars; problem q's
    // num_vis is its observation count obs_ptr[q + 1] - obs_ptr[q]
    void apply(const double *out, const long long *obs_ptr)
    {
        for (size_t q = 0; q < np; q++) {
            if (!active[q]) continue;   // a finished problem keeps its last flags
            accepted_prev[q] = 0;
            relin[q] = 0;
            const double old = out[4 * q], nw = out[4 * q + 1], dpg = out[4 * q + 2];
            const double num_vis = (double)(obs_ptr[q + 1] - obs_ptr[q]);
            const double rho = (old - nw) / dpg;
            passes[q]++;
            total_passes++;
            if ((old - nw) > 0) {   // bundle_euclid.m:218-232
                const double olde = old / num_vis, newe = nw / num_vis;
                if ((int)err[q].size() < iter[q]) err[q].push_back(olde);
                else err[q][iter[q] - 1] = olde;
                iter[q]++;
                err[q].push_back(newe);
                iter2[q] = 0;
                lam[q] = lam[q] * std::max(1.0 / 3.0, 1.0 - std::pow(2.0 * rho - 1.0, 3));
                nu[q] = 2.0;
                accepted_prev[q] = 1;
                relin[q] = 1;
                acc[q]++;
                total_acc++;
            } else {                // :233-241
                lam[q] = lam[q] * nu[q];
                nu[q] = 2.0 * nu[q];
                iter2[q]++;
            }
        }
    }

    // row q of error_out (np x error_cap) = problem q's error_
    void write_errors(double *error_out, int error_cap, int *num_error) const
    {
        for (size_t q = 0; q < np; q++) {
            if (num_error) num_error[q] = (int)err[q].size();
            if (error_out)
                for (size_t k = 0; k < err[q].size() && k < (size_t)error_cap; k++)
                    error_out[(size_t)error_cap * q + k] = err[q][k];
        }
    }

    void fill_stats(vlgba_stats *stats, std::chrono::steady_clock::time_point t0) const
    {
        if (!stats) return;
        stats->iterations = total_passes;
        stats->accepted = total_acc;
        stats->num_error = 0;
        stats->lambda = np ? lam[0] : 0.0;
        stats->pinv_passes = stats->spin_retries = stats->nd_retries = 0;
        stats->seconds =
            std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    }
};
