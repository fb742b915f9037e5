// sk.h -- launch interface of the spectral kurtosis cascade's segment kernel (sk.hip).  The jobs are the pair object's (cross.h)
// with src[0] only: one real stream a unit.  A workgroup's partial is 2 rows of n/2 + 1: S1 = sum w P and S2 = sum w P^2 of the
// periodogram P = |X|^2 (sk_fft.h).  Decimator, fold and tails are those of the pair object.
#pragma once
#include "cross.h"

namespace psdk {

int sk_segments_per_tile(int n);
hipError_t launch_sk(int n, const CrossBatch &b, const float *win, const cf *tw, hipStream_t s);

} // namespace psdk
