// longqc_amd/csrc/figdata_dev.hpp -- figdata.cpp's histogram and log-sum passes over an array that already lies on the device (the
// kernels of kernels_figdata.hpp are compiled in figdata.cpp alone).  Both wait for the stream; the caller has checked the arguments:
// n >= 1 values, n_edges >= 2 ascending edges.
#pragma once
#include "lq_cabi.hpp"

void lq_fig_hist_dev(hipStream_t s, int dtype, const void *d_x, u64 n, const double *edges, u32 n_edges, u64 *counts);
void lq_fig_logsum_dev(hipStream_t s, const u32 *d_x, u64 n, uint64_t *sum, double *sum_log, uint64_t *n_zero);
