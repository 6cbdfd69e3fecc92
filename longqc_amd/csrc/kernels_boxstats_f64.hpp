// longqc_amd/csrc/kernels_boxstats_f64.hpp -- box-plot statistics by group over doubles: df.boxplot(column='ReadScore', by='Interval') of
// lq_rs.py:17-19, which is matplotlib.cbook.boxplot_stats per group.  The thousandths entry (kernels_boxstats.hpp) stays as it is; this is
// a second body with the same order statistics, the same _lerp rule, whisker fallback and flier counts and the same LQ_BOX_* macros (no
// fused arithmetic), on values that are loaded as doubles.  The host side is boxstats_f64.cpp, which includes kernels_boxstats.hpp first.
//
//   k_boxd_keys    per element the value's order key -- its bit pattern with the sign corrected: ascending keys are ascending doubles,
//                  -0.0 in front of +0.0 -- its index, and its group: key[i], or floor((double)key[i] / interval) by the IEEE division.
//                  err |= 1 for a NaN, 2 for a group of 2^32 or more; the largest group by atomicMax.
//   (the sorts)    two stable passes of Prim::radix, as k_pol_* orders its items: by value over 64 bits, then (k_boxd_rekey) by group
//                  over the bits the largest group has.  Integers: the same bytes from every run.
//   k_boxd_flags   sorted[i] = x[idx[i]], flag[i] = 1 where the group changes (flag[n] = 0).
//   k_box_heads    (kernels_boxstats.hpp) head[g] = the first element of group g.
//   k_boxd_stats   one thread per group, as k_box_stats.  There are no missing values: n = n_all.
#pragma once
#include <cmath>

// lqfig_box_f64 of include/lqcov.h, field for field (boxstats_f64.cpp asserts the size)
struct LqBoxD {
	u32 group, reserved;
	u64 first, n_all, n;
	double mid_lo, mid_hi;
	double q1, med, q3, whislo, whishi;
	u64 n_low, n_high;
};

__device__ __forceinline__ u64 lq_boxd_key(double x)
{
	u64 b;
	__builtin_memcpy(&b, &x, 8);
	return b >> 63 ? ~b : b | 0x8000000000000000ULL;
}

// ctl[0] = the largest group (the host zeroes it), ctl[1] |= the refusals
static __global__ void __launch_bounds__(LQ_BOX_THREADS)
k_boxd_keys(const u32 *key, const double *x, u64 n, double interval, u64 *vk, u64 *idx, u32 *grp, u32 *ctl)
{
	u32 gmax = 0, err = 0;
	for (u64 i = (u64)blockIdx.x * LQ_BOX_THREADS + threadIdx.x; i < n; i += (u64)gridDim.x * LQ_BOX_THREADS) {
		u32 g = key[i];
		if (interval != 0.0) {
			const double b = floor(LQ_BOX_DIV((double)g, interval));
			if (b >= 4294967296.0) { err |= 2u; g = 0; } else g = (u32)b;
		}
		const double v = x[i];
		if (v != v) err |= 1u;
		vk[i] = lq_boxd_key(v); idx[i] = i; grp[i] = g;
		gmax = g > gmax ? g : gmax;
	}
	if (gmax) atomicMax(ctl, gmax);
	if (err) atomicOr(ctl + 1, err);
}

// g2[i] = grp[idx[i]]: the second pass's keys in the first pass's order
static __global__ void __launch_bounds__(LQ_BOX_THREADS)
k_boxd_rekey(const u32 *grp, const u64 *idx, u64 n, u32 *g2)
{
	for (u64 i = (u64)blockIdx.x * LQ_BOX_THREADS + threadIdx.x; i < n; i += (u64)gridDim.x * LQ_BOX_THREADS) g2[i] = grp[idx[i]];
}

// gs: the groups in sorted order; flag has n + 1 entries
static __global__ void __launch_bounds__(LQ_BOX_THREADS)
k_boxd_flags(const u32 *gs, const u64 *idx, const double *x, u64 n, double *sorted, u32 *flag)
{
	for (u64 i = (u64)blockIdx.x * LQ_BOX_THREADS + threadIdx.x; i <= n; i += (u64)gridDim.x * LQ_BOX_THREADS) {
		if (i == n) { flag[i] = 0; continue; }
		sorted[i] = x[idx[i]];
		flag[i] = i == 0 || gs[i - 1] != gs[i] ? 1u : 0u;
	}
}

// np.percentile's linear rule on s[0..n), n >= 1, ascending: q = num / 4
__device__ __forceinline__ double lq_boxd_quantile(const double *s, u64 n, u32 num)
{
	const double vi = LQ_BOX_MUL((double)(n - 1), 0.25 * num);    // (exact below 2^51)
	const double fl = floor(vi), t = LQ_BOX_SUB(vi, fl);
	const u64 lo = (u64)fl, hi = lo + 1 < n ? lo + 1 : n - 1;
	const double a = s[lo], b = s[hi], d = LQ_BOX_SUB(b, a);
	if (t >= 0.5) return LQ_BOX_SUB(b, LQ_BOX_MUL(d, LQ_BOX_SUB(1.0, t)));
	return LQ_BOX_ADD(a, LQ_BOX_MUL(d, t));
}

// the values of s[0..n) below x (strict: the first at or above it), or at or below x
__device__ __forceinline__ u64 lq_boxd_count(const double *s, u64 n, double x, bool or_equal)
{
	u64 lo = 0, hi = n;
	while (lo < hi) {
		const u64 mid = lo + (hi - lo) / 2;
		const double v = s[mid];
		if (or_equal ? v <= x : v < x) lo = mid + 1; else hi = mid;
	}
	return lo;
}

static __global__ void __launch_bounds__(LQ_BOX_THREADS)
k_boxd_stats(const u32 *gs, const double *sorted, const u32 *head, u32 n_groups, double whis, LqBoxD *box)
{
	for (u64 g = (u64)blockIdx.x * LQ_BOX_THREADS + threadIdx.x; g < n_groups; g += (u64)gridDim.x * LQ_BOX_THREADS) {
		const u64 first = head[g], n = head[g + 1] - first;
		const double *s = sorted + first;
		LqBoxD b;
		b.group = gs[first]; b.reserved = 0;
		b.first = first; b.n_all = n; b.n = n;
		b.mid_lo = s[(n - 1) / 2]; b.mid_hi = s[n / 2];
		b.q1 = lq_boxd_quantile(s, n, 1); b.med = lq_boxd_quantile(s, n, 2); b.q3 = lq_boxd_quantile(s, n, 3);
		const double reach = LQ_BOX_MUL(whis, LQ_BOX_SUB(b.q3, b.q1));
		const u64 n_le = lq_boxd_count(s, n, LQ_BOX_ADD(b.q3, reach), true);      // the values at or below q3 + whis iqr
		double w = n_le ? s[n_le - 1] : b.q3;
		b.whishi = w < b.q3 ? b.q3 : w;
		const u64 n_lt = lq_boxd_count(s, n, LQ_BOX_SUB(b.q1, reach), false);     // the values below q1 - whis iqr
		w = n_lt < n ? s[n_lt] : b.q1;
		b.whislo = w > b.q1 ? b.q1 : w;
		b.n_low = lq_boxd_count(s, n, b.whislo, false);
		b.n_high = n - lq_boxd_count(s, n, b.whishi, true);
		box[g] = b;
	}
}
