// longqc_amd/csrc/boxstats_dev.hpp -- boxstats_f64.cpp's pass over a key array and a value array that already lie on the device (its
// kernels are compiled in boxstats_f64.cpp alone).  It checks interval, whis and n as lqfig_boxstats_f64 states them, waits for the
// stream, and writes sorted (n doubles) and the boxes to the host.
#pragma once
#include "lq_cabi.hpp"

void lq_box_f64_dev(hipStream_t s, const u32 *d_key, const double *d_x, u64 n, double interval, double whis, double *sorted, lqfig_box_f64 *boxes,
                    u32 box_cap, u32 *n_boxes);
