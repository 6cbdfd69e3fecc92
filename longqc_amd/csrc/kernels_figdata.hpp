// longqc_amd/csrc/kernels_figdata.hpp -- the numbers behind LongQC's two distribution figures, over every read of a run: the
// histograms and Gaussian KDE curves of plot_unmasked_gc_frac (lq_gcfrac.py:49-85) and the length histogram and the sums of the gamma
// fit (lq_gamma.py:47-59, longQC.py:487-488).  Nothing is drawn; the host side is figdata.cpp, the caller longqc_amd/figdata.py.
//
//   k_fig_range   min and max of a float32 / uint32 array as order-preserving 32-bit keys (integer atomicMin / atomicMax; NaN skipped).
//   k_fig_hist    np.histogram(a, bins=edges) for an explicit edge array, numpy's rule: bin k counts edges[k] <= v < edges[k+1], the
//                 last bin is closed on the right, a value outside [edges[0], edges[-1]] or NaN is counted nowhere.  Every element is
//                 converted to double exactly and its bin settled by bisecting the edge array itself (np.arange's edges are not
//                 e0 + k w in exact arithmetic).  Up to LQ_FIG_HIST_LDS_BINS bins: edges and block-private u32 counters in LDS,
//                 flushed with 64-bit global atomics; more bins: the edges are read from global memory, one global atomic per value.
//   k_fig_kde     S[j] = sum_i exp(-0.5 u u), u = (p[j] - d[i]) / h in double, the difference first.  THE FOLDING RULE, shared with
//                 k_fig_logsum: the data are cut into tiles of LQ_FIG_TILE = 256 values, tile t = [256 t, min(n, 256 t + 256)), a function
//                 of n alone.  A wave takes a tile, lane j owns point j (64 points at a time), reads the tile's data wave-uniformly and
//                 adds its point's terms in index order; the partial goes to part[t][j].  k_fig_fold then folds the [tile][m] array over the
//                 tile index in a fixed pairwise tree (node q of level k = tiles [q 2^k, (q+1) 2^k), a missing child = +0.0, which is exact
//                 here: x + 0.0 == x for every x but -0.0, and no partial is -0.0).  No floating-point atomics, no cross-lane sum: the result does
//                 not depend on the grid, on the run, or on which wave finishes first.
//   k_fig_logsum  for a uint32 array: sum x (u64) and the number of zeros by integer atomics, and sum log(x) over the non-zero values
//                 under the same rule: lane l of a tile's wave adds log of values 4 l .. 4 l + 3 in index order, the 64 lane sums are folded
//                 by the butterfly below (a fixed tree over the lane index), part[t] goes to k_fig_fold with m = 1.
//   k_fig_fold    one level of radix 8 = three levels of the pairwise tree: out[q][j] = ((a0 + a1) + (a2 + a3)) + ((a4 + a5) + (a6 + a7)),
//                 a_i = in[8 q + i][j] (0.0 behind the last row).
#pragma once
#include "lq_common.hpp"
#include <cmath>

#define LQ_FIG_THREADS 256
#define LQ_FIG_MAX_BLOCKS 1024u      // elements / tiles are strided over the blocks of a launch
#define LQ_FIG_TILE 256u             // values of one tile: at most 256 terms are added one after the other
#define LQ_FIG_HIST_LDS_BINS 1024u   // bins whose edges and counters fit a block's LDS: (1025 x 8 + 1024 x 4) bytes
#ifndef LQ_FIG_LAST_BIN_CLOSED
#define LQ_FIG_LAST_BIN_CLOSED 1     // numpy's rule.  0: the last bin half-open like the others -- the slip tests/test_figdata_hist.py builds once to see it noticed
#endif

// order-preserving u32 key of a float32 (k_fig_range); uint32 values are their own keys
__host__ __device__ __forceinline__ u32 lq_fig_key(u32 bits) { return bits & 0x80000000u ? ~bits : bits | 0x80000000u; }
__host__ __device__ __forceinline__ u32 lq_fig_unkey(u32 key) { return key & 0x80000000u ? key & 0x7fffffffu : ~key; }

__device__ __forceinline__ double lq_fig_value(const float *x, u64 i) { return (double)x[i]; }
__device__ __forceinline__ double lq_fig_value(const u32 *x, u64 i) { return (double)x[i]; }

// mm[0] = min key, mm[1] = max key (the host sets 0xffffffff / 0); is_float: x holds float32 bit patterns, NaN is skipped
__global__ void __launch_bounds__(LQ_FIG_THREADS)
k_fig_range(const u32 *x, u64 n, int is_float, u32 *mm)
{
	u32 lo = 0xffffffffu, hi = 0;
	for (u64 i = (u64)blockIdx.x * LQ_FIG_THREADS + threadIdx.x; i < n; i += (u64)gridDim.x * LQ_FIG_THREADS) {
		const u32 b = x[i];
		if (is_float && (b & 0x7fffffffu) > 0x7f800000u) continue;
		const u32 k = is_float ? lq_fig_key(b) : b;
		lo = k < lo ? k : lo; hi = k > hi ? k : hi;
	}
	if (lo <= hi) { atomicMin(mm, lo); atomicMax(mm + 1, hi); }
}

// the bin of v among e[0..nb] (ascending, nb >= 1), or nb when v is counted nowhere: the last k with e[k] <= v, the last edge into bin nb - 1
__device__ __forceinline__ u32 lq_fig_bin(const double *e, u32 nb, double v)
{
	if (!(v >= e[0]) || !(v <= e[nb])) return nb;             // (NaN fails both)
	u32 lo = 0, hi = nb;                                      // invariant: e[lo] <= v, and e[hi + 1] > v or hi == nb
	while (lo < hi) {
		const u32 mid = lo + (hi - lo + 1) / 2;
		if (e[mid] <= v) lo = mid; else hi = mid - 1;
	}
	return lo == nb ? (LQ_FIG_LAST_BIN_CLOSED ? nb - 1 : nb) : lo;
}

// counts[k] += the values of x[0..n) in bin k of edges[0..n_edges) (n_edges >= 2); counts is zeroed by the host
template <class T> __global__ void __launch_bounds__(LQ_FIG_THREADS)
k_fig_hist(const T *x, u64 n, const double *edges, u32 n_edges, unsigned long long *counts)
{
	__shared__ double s_e[LQ_FIG_HIST_LDS_BINS + 1];
	__shared__ u32 s_c[LQ_FIG_HIST_LDS_BINS];
	const u32 nb = n_edges - 1;
	const u64 first = (u64)blockIdx.x * LQ_FIG_THREADS + threadIdx.x, step = (u64)gridDim.x * LQ_FIG_THREADS;
	if (nb > LQ_FIG_HIST_LDS_BINS) {                          // (the same for the whole launch)
		for (u64 i = first; i < n; i += step) {
			const u32 k = lq_fig_bin(edges, nb, lq_fig_value(x, i));
			if (k < nb) atomicAdd(counts + k, 1ULL);
		}
		return;
	}
	for (u32 k = threadIdx.x; k <= nb; k += LQ_FIG_THREADS) s_e[k] = edges[k];
	for (u32 k = threadIdx.x; k < nb; k += LQ_FIG_THREADS) s_c[k] = 0;
	__syncthreads();
	for (u64 i = first; i < n; i += step) {
		const u32 k = lq_fig_bin(s_e, nb, lq_fig_value(x, i));
		if (k < nb) atomicAdd(s_c + k, 1u);                   // (a block sees fewer than 2^32 values: the host takes no more per call)
	}
	__syncthreads();
	for (u32 k = threadIdx.x; k < nb; k += LQ_FIG_THREADS)
		if (s_c[k]) atomicAdd(counts + k, (unsigned long long)s_c[k]);
}

// part[t * m + j] = the terms of point j over tile t, added in index order (the folding rule above)
__global__ void __launch_bounds__(LQ_FIG_THREADS)
k_fig_kde(const float *d, u64 n, const double *p, u32 m, double h, double *part)
{
	const u32 lane = threadIdx.x & 63;
	const u64 n_tiles = (n + LQ_FIG_TILE - 1) / LQ_FIG_TILE;
	const u64 wave = (u64)blockIdx.x * (LQ_FIG_THREADS / 64) + threadIdx.x / 64, n_waves = (u64)gridDim.x * (LQ_FIG_THREADS / 64);
	for (u64 t = wave; t < n_tiles; t += n_waves) {
		const u64 i0 = t * LQ_FIG_TILE;
		const u32 cnt = (u32)(n - i0 < LQ_FIG_TILE ? n - i0 : LQ_FIG_TILE);
		for (u32 j = lane; j < m; j += 64) {
			const double pj = p[j];
			double acc = 0.0;
			for (u32 i = 0; i < cnt; ++i) {                        // (d[i0 + i]: one address for the wave)
				const double u = (pj - (double)d[i0 + i]) / h;
				acc += exp(-0.5 * u * u);
			}
			part[t * m + j] = acc;
		}
	}
}

// tot[0] += sum x, tot[1] += the zeros; part[t] = sum of log(x) over the non-zero values of tile t
__global__ void __launch_bounds__(LQ_FIG_THREADS)
k_fig_logsum(const u32 *x, u64 n, unsigned long long *tot, double *part)
{
	const u32 lane = threadIdx.x & 63;
	const u64 n_tiles = (n + LQ_FIG_TILE - 1) / LQ_FIG_TILE;
	const u64 wave = (u64)blockIdx.x * (LQ_FIG_THREADS / 64) + threadIdx.x / 64, n_waves = (u64)gridDim.x * (LQ_FIG_THREADS / 64);
	unsigned long long sum = 0, zeros = 0;
	for (u64 t = wave; t < n_tiles; t += n_waves) {             // (wave-uniform: the shuffles below run converged)
		const u64 i0 = t * LQ_FIG_TILE + 4 * lane;
		double s = 0.0;
		for (u32 i = 0; i < 4; ++i) {
			if (i0 + i >= n) break;
			const u32 v = x[i0 + i];
			sum += v;
			if (v) s += log((double)v); else ++zeros;
		}
		for (int o = 1; o < 64; o <<= 1) {                        // lanes (2 o) q and (2 o) q + o: a pairwise tree over the lane index
			s += __shfl_xor(s, o);                                // (both lanes of a pair get the same sum: a + b == b + a)
		}
		if (lane == 0) part[t] = s;
	}
	if (sum) atomicAdd(tot, sum);
	if (zeros) atomicAdd(tot + 1, zeros);
}

// out[q * m + j] = the pairwise sum of in[(8 q .. 8 q + 7) * m + j], rows at or behind `rows` read as 0.0
__global__ void __launch_bounds__(LQ_FIG_THREADS)
k_fig_fold(const double *in, u64 rows, u32 m, double *out)
{
	const u64 n_out = (rows + 7) / 8 * m;
	for (u64 g = (u64)blockIdx.x * LQ_FIG_THREADS + threadIdx.x; g < n_out; g += (u64)gridDim.x * LQ_FIG_THREADS) {
		const u64 q = g / m, j = g % m;
		double a[8];
		for (u32 i = 0; i < 8; ++i) a[i] = 8 * q + i < rows ? in[(8 * q + i) * m + j] : 0.0;
		out[g] = ((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7]));
	}
}
