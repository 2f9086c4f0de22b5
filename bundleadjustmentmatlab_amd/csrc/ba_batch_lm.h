// ba_batch_lm.h -- the batched one-block LM, host only: the LM control of
// bundle_euclid.m:120-123, 205-241 applied per problem, each with its own lambda
// (batch_lm), and the loop that drives a backend with it (batch_lm_run).  No
// HIP here: vlgba_resect[_ex] (ba_resect.hip: one camera, structure fixed) and
// vlgba_intersect[_ex] (ba_triang.hip: one point, motion fixed) run it on the
// device backend of ba_batch_dev.h, tests/native/block_host.cpp on a CPU one.
//
// Protocol of a pass, the contract between the driver and a backend.  The driver
// owns a staging block of 6 np doubles, lam [np] | flags [np] | out [4 np]
// (flags == lam + np: a backend may move both in one copy).  stage() decides
// which problems go on (:120-123) and writes lambda and the flags word of every
// problem, as doubles; backend.pass(lam, flags, out) runs every problem whose
// flags has bit 1 and writes four doubles for it -- old cost, new cost,
// dp'(lambda dp + g), 1.0 if the step came from the pinv fallback else 0.0 --
// leaving the four of a finished problem alone; apply() applies :218-241.  The
// backend keeps two parameter sets per problem, x (the linearisation point) and
// x_new (the last step's), and takes x_new as x first when told that the
// previous pass was accepted; after the last pass backend.fetch hands back both
// and the driver picks.  Under a loss the pass reports the robust cost and
// gradient in the same places; nothing here changes.
//   flags: 1 active | 2 linearise again (the parameters changed) | 4 the
//          previous pass was accepted (take x_new as x first)
#pragma once
#include "../../include/vlgba.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <vector>

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
    int total_passes = 0, total_acc = 0, total_pinv = 0;

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
            total_pinv += out[4 * q + 3] != 0.0;   // the step came from the pinv fallback
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
        stats->pinv_passes = total_pinv;
        stats->spin_retries = stats->nd_retries = 0;
        stats->seconds =
            std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    }
};

// what runs the passes of np problems with nx parameters each (protocol above);
// both return 0 or an error code, which ends the solve
struct batch_backend {
    virtual ~batch_backend() = default;
    virtual int pass(const double *lam, const double *flags, double *out) = 0;
    virtual int fetch(double *x, double *x_new) = 0;   // nx * np doubles each
};

// The LM of every problem of lm on be: x (nx * np) receives the parameters of
// the last accepted step, error_out / num_error as write_errors, stats as
// fill_stats (pinv_passes: the passes whose fourth scalar was set; apply() counts
// them while it has the pass's scalars in hand -- a loop of its own here put
// vlgba_intersect on 20 000 points 3 % above its time, profiles/block_host/).
// stage: 6 np doubles.
inline int batch_lm_run(batch_lm &lm, batch_backend &be, double *stage, int nx,
                        const long long *obs_ptr, double *x, double *error_out, int error_cap,
                        int *num_error, vlgba_stats *stats,
                        std::chrono::steady_clock::time_point t0)
{
    const size_t np = lm.np;
    double *lam = stage, *flags = stage + np, *out = stage + 2 * np;
    int rc = 0;
    while (!rc && lm.stage(lam, flags))
        if (!(rc = be.pass(lam, flags, out))) lm.apply(out, obs_ptr);
    std::vector<double> xn((size_t)nx * np);
    if (!rc && !(rc = be.fetch(x, xn.data()))) {
        for (size_t q = 0; q < np; q++)   // the last accepted step's parameters
            if (lm.accepted_prev[q])
                std::memcpy(x + (size_t)nx * q, xn.data() + (size_t)nx * q, sizeof(double) * nx);
        lm.write_errors(error_out, error_cap, num_error);
    }
    lm.fill_stats(stats, t0);
    return rc;
}
