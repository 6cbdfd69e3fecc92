// longqc_amd/csrc/kernels_boxstats.hpp -- box-plot statistics by group, over every read of a run: what LongQC's three grouped box plots
// compute before they draw (the QV by length bin of lq_mask.py:43-79, the coverage by length bin of lq_coverage.py:462-529, the QV by
// "coverage is zero or not" of lq_coverage.py:438-460).  Nothing is drawn; the host side is boxstats.cpp, the caller longqc_amd/figdata.py.
//
// A value is a printed "%.3f" number, an integer count of thousandths (lq_fmt3.hpp); its double is thou / 1000, one IEEE division,
// which is float(text).  LQ_BOX_MISSING (INT32_MIN) is "-nan".  A group's box is matplotlib.cbook.boxplot_stats(x, whis) on its
// non-missing values: np.percentile's linear rule, the whiskers' fallback to the quartile, the fliers as two stretches of the sorted values.
//
//   k_box_keys    per element the 64-bit key group << 32 | value with the sign bit flipped (ascending keys = ascending values inside a
//                 group), a missing value as 0xffffffff: last in its group.  group = key[i], or floor((double)key[i] / interval): the IEEE
//                 division, not a product with the reciprocal (49 * (1 / 49.0) < 1).  The largest group by integer atomicMax: the sort then
//                 runs over 32 + its bits only.  err |= 1 for a value that is INT32_MAX (its key is the missing one), 2 for a group of
//                 2^32 or more.
//   (the sort)    Prim::radix on the keys alone (kernels_isort.hpp): integers, so the same bytes from every run.
//   k_box_flags   from the sorted keys: sorted[i] = the value back as thousandths, flag[i] = 1 where key >> 32 changes (flag[n] = 0, for the
//                 scan of n + 1 entries whose last is the number of groups).
//   k_box_heads   head[pos[i]] = i where flag[i], head[groups] = n: group g is sorted[head[g] .. head[g + 1]).
//   k_box_stats   one thread per group: n by bisection for the first missing value, the order statistics, the two interpolations, the two
//                 whisker searches and the two flier counts by bisection in the group's stretch.  A group costs O(log n) loads; a wave per
//                 group would leave 63 lanes idle in every bisection.
// NO FUSED ARITHMETIC: numpy rounds every operation of a + (b - a) * t on its own, hipcc contracts it into a fused multiply-add by
// default.  Every double operation here goes through LQ_BOX_MUL / ADD / SUB / DIV: the __d*_rn intrinsics, which never fuse; plain
// operators in the emulator build (x86-64 without FMA code generation).
#pragma once
#include "lq_common.hpp"
#include <cmath>

#define LQ_BOX_THREADS 256
#define LQ_BOX_MAX_BLOCKS 64u        // elements / groups are strided over the blocks of a launch: 16384 a round
#define LQ_BOX_MISSING ((i32)0x80000000)
#ifndef LQ_BOX_LERP_TWO_SIDED
#define LQ_BOX_LERP_TWO_SIDED 1      // numpy's _lerp: b - (b - a) * (1 - t) where t >= 0.5.  0: a + (b - a) * t for every t -- a slip tests/test_boxstats.py builds once to see it noticed
#endif
#ifndef LQ_BOX_BIN_BY_DIVISION
#define LQ_BOX_BIN_BY_DIVISION 1     // np.floor(len / interval).  0: floor(len * (1 / interval)) -- the other slip built there
#endif

#ifndef LQ_EMU
#define LQ_BOX_MUL(a, b) __dmul_rn((a), (b))
#define LQ_BOX_ADD(a, b) __dadd_rn((a), (b))
#define LQ_BOX_SUB(a, b) __dsub_rn((a), (b))
#define LQ_BOX_DIV(a, b) __ddiv_rn((a), (b))
#else
#define LQ_BOX_MUL(a, b) ((a) * (b))
#define LQ_BOX_ADD(a, b) ((a) + (b))
#define LQ_BOX_SUB(a, b) ((a) - (b))
#define LQ_BOX_DIV(a, b) ((a) / (b))
#endif

// lqfig_box of include/lqcov.h, field for field (boxstats.cpp asserts the size)
struct LqBox {
	u32 group, reserved;
	u64 first, n_all, n;
	i32 mid_lo, mid_hi;
	double q1, med, q3, whislo, whishi;
	u64 n_low, n_high;
};

__device__ __forceinline__ double lq_box_value(i32 thou) { return LQ_BOX_DIV((double)thou, 1000.0); }

// ctl[0] = the largest group (the host zeroes it), ctl[1] |= the refusals
__global__ void __launch_bounds__(LQ_BOX_THREADS)
k_box_keys(const u32 *key, const i32 *thou, u64 n, double interval, u64 *out, u32 *ctl)
{
	u32 gmax = 0, err = 0;
	for (u64 i = (u64)blockIdx.x * LQ_BOX_THREADS + threadIdx.x; i < n; i += (u64)gridDim.x * LQ_BOX_THREADS) {
		u32 g = key[i];
		if (interval != 0.0) {
#if LQ_BOX_BIN_BY_DIVISION
			const double b = floor(LQ_BOX_DIV((double)g, interval));
#else
			const double b = floor(LQ_BOX_MUL((double)g, LQ_BOX_DIV(1.0, interval)));
#endif
			if (b >= 4294967296.0) { err |= 2u; g = 0; } else g = (u32)b;
		}
		const i32 v = thou[i];
		if (v == 0x7fffffff) err |= 1u;
		const u32 low = v == LQ_BOX_MISSING ? 0xffffffffu : (u32)v ^ 0x80000000u;
		out[i] = (u64)g << 32 | low;
		gmax = g > gmax ? g : gmax;
	}
	if (gmax) atomicMax(ctl, gmax);
	if (err) atomicOr(ctl + 1, err);
}

// flag has n + 1 entries
__global__ void __launch_bounds__(LQ_BOX_THREADS)
k_box_flags(const u64 *k, u64 n, i32 *sorted, u32 *flag)
{
	for (u64 i = (u64)blockIdx.x * LQ_BOX_THREADS + threadIdx.x; i <= n; i += (u64)gridDim.x * LQ_BOX_THREADS) {
		if (i == n) { flag[i] = 0; continue; }
		const u64 x = k[i];
		const u32 low = (u32)x;
		sorted[i] = low == 0xffffffffu ? LQ_BOX_MISSING : (i32)(low ^ 0x80000000u);
		flag[i] = i == 0 || (u32)(k[i - 1] >> 32) != (u32)(x >> 32) ? 1u : 0u;
	}
}

// pos: the exclusive scan of flag over n + 1 entries (pos[n] = the groups); head has pos[n] + 1 entries
__global__ void __launch_bounds__(LQ_BOX_THREADS)
k_box_heads(const u32 *flag, const u32 *pos, u64 n, u32 *head)
{
	for (u64 i = (u64)blockIdx.x * LQ_BOX_THREADS + threadIdx.x; i < n; i += (u64)gridDim.x * LQ_BOX_THREADS) {
		if (flag[i]) head[pos[i]] = (u32)i;
		if (i + 1 == n) head[pos[n]] = (u32)n;
	}
}

// np.percentile's linear rule on s[0..n), n >= 1, ascending thousandths: q = num / 4
__device__ __forceinline__ double lq_box_quantile(const i32 *s, u64 n, u32 num)
{
	const double vi = LQ_BOX_MUL((double)(n - 1), 0.25 * num);    // (exact below 2^51)
	const double fl = floor(vi), t = LQ_BOX_SUB(vi, fl);
	const u64 lo = (u64)fl, hi = lo + 1 < n ? lo + 1 : n - 1;
	const double a = lq_box_value(s[lo]), b = lq_box_value(s[hi]), d = LQ_BOX_SUB(b, a);
#if LQ_BOX_LERP_TWO_SIDED
	if (t >= 0.5) return LQ_BOX_SUB(b, LQ_BOX_MUL(d, LQ_BOX_SUB(1.0, t)));
#endif
	return LQ_BOX_ADD(a, LQ_BOX_MUL(d, t));
}

// the values of s[0..n) below x (strict: the first at or above it), or at or below x
__device__ __forceinline__ u64 lq_box_count(const i32 *s, u64 n, double x, bool or_equal)
{
	u64 lo = 0, hi = n;
	while (lo < hi) {
		const u64 mid = lo + (hi - lo) / 2;
		const double v = lq_box_value(s[mid]);
		if (or_equal ? v <= x : v < x) lo = mid + 1; else hi = mid;
	}
	return lo;
}

__global__ void __launch_bounds__(LQ_BOX_THREADS)
k_box_stats(const u64 *k, const i32 *sorted, const u32 *head, u32 n_groups, double whis, LqBox *box)
{
	for (u64 g = (u64)blockIdx.x * LQ_BOX_THREADS + threadIdx.x; g < n_groups; g += (u64)gridDim.x * LQ_BOX_THREADS) {
		const u64 first = head[g], n_all = head[g + 1] - first;
		const i32 *s = sorted + first;
		u64 lo = 0, hi = n_all;                                   // the first missing value: they are last in the group
		while (lo < hi) {
			const u64 mid = lo + (hi - lo) / 2;
			if (s[mid] != LQ_BOX_MISSING) lo = mid + 1; else hi = mid;
		}
		const u64 n = lo;
		LqBox b;
		b.group = (u32)(k[first] >> 32); b.reserved = 0;
		b.first = first; b.n_all = n_all; b.n = n;
		if (n == 0) {
			b.mid_lo = b.mid_hi = LQ_BOX_MISSING;
			b.q1 = b.med = b.q3 = b.whislo = b.whishi = NAN;
			b.n_low = b.n_high = 0;
			box[g] = b;
			continue;
		}
		b.mid_lo = s[(n - 1) / 2]; b.mid_hi = s[n / 2];
		b.q1 = lq_box_quantile(s, n, 1); b.med = lq_box_quantile(s, n, 2); b.q3 = lq_box_quantile(s, n, 3);
		const double reach = LQ_BOX_MUL(whis, LQ_BOX_SUB(b.q3, b.q1));
		const u64 n_le = lq_box_count(s, n, LQ_BOX_ADD(b.q3, reach), true);       // the values at or below q3 + whis iqr
		double w = n_le ? lq_box_value(s[n_le - 1]) : b.q3;
		b.whishi = w < b.q3 ? b.q3 : w;
		const u64 n_lt = lq_box_count(s, n, LQ_BOX_SUB(b.q1, reach), false);      // the values below q1 - whis iqr
		w = n_lt < n ? lq_box_value(s[n_lt]) : b.q1;
		b.whislo = w > b.q1 ? b.q1 : w;
		b.n_low = lq_box_count(s, n, b.whislo, false);
		b.n_high = n - lq_box_count(s, n, b.whishi, true);
		box[g] = b;
	}
}
