// ba_batch_dev.h -- the device side of the batched one-block LM (ba_batch_lm.h),
// shared by vlgba_resect[_ex] (ba_resect.hip) and vlgba_intersect[_ex]
// (ba_triang.hip): the pooled stream and pinned block of a call, and the backend
// that owns x | x_new, lam | flags and out on the device and runs the copy,
// launch, copy, synchronise of one pass around the entry's own launch.
#pragma once
#include "ba_batch_lm.h"
#include "ba_internal.h"

#include <functional>

// A stream and a pinned host block (>= need doubles) from the per-device pool,
// held for one call and given back, drained, on every path: creating a stream
// and pageable copies cost more than the resection itself (the growing-BA replay
// calls it once per added camera).  Declare the device buffers used on s BEFORE
// the guard: they are then freed after it has drained the stream.
struct batch_stream {
    int rc;   // 0, or the error of the acquisition (use nothing then)
    hipStream_t s = nullptr;
    double *pin = nullptr;
    batch_stream(int device, size_t need);
    ~batch_stream();
    batch_stream(const batch_stream &) = delete;
    batch_stream &operator=(const batch_stream &) = delete;

private:
    int device_;
    size_t cap_ = 0;
};

// the device pointers of a pass (the protocol of ba_batch_lm.h): nx doubles per
// problem in x and x_new, np in lam and flags, 4 np in out
struct batch_dev_io {
    double *x, *x_new;
    const double *lam, *flags;
    double *out;
};
// an entry's launch on bs.s: 0 or an error code
using batch_dev_fn = std::function<int(const batch_dev_io &)>;

// batch_lm_run on the device: uploads x (nx per problem), runs pass once per LM
// pass, leaves the result in x; then, unless empty, residuals with io.x at the
// returned parameters (what it queues on bs.s has completed on return).
int batch_dev_run(batch_stream &bs, batch_lm &lm, int nx, const long long *obs_ptr, double *x,
                  double *error_out, int error_cap, int *num_error, vlgba_stats *stats,
                  std::chrono::steady_clock::time_point t0, const batch_dev_fn &pass,
                  const batch_dev_fn &residuals);
