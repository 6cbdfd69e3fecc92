// longqc_amd/csrc/kernels_mixfit.hpp -- the two mixture fits behind LqCoverage's coverage estimate (lq_coverage.py:552-621), each a whole EM
// loop in one launch: one workgroup per fit, the stopping rule on the device.  The host side is mixfit.cpp, the caller longqc_amd/mixfit.py.
//
//   k_mix_gmm2     sklearn's 1-D two-component GaussianMixture.fit after its initialisation (sklearn/mixture/_base.py fit_predict,
//                  _gaussian_mixture.py, covariance_type "full"): an M-step from one-hot responsibilities (the first `split` values of the
//                  ascending segment are component 0), then E-step / M-step / lower bound until |bound - previous| < tol or max_iter.
//   k_mix_lognorm  mixem.em for [NormalDistribution, LogNormalDistribution] (mixEM/mixem/em.py:33-88): initial weights (1, 1), its three
//                  exits in its order.  A NaN log-likelihood is reported as it is (exit LQ_MIX_EXIT_NAN), not repaired.
//
// WHO ADDS WHAT.  Every sum over the data follows kernels_figdata.hpp's folding rule: tiles of LQ_MIX_TILE = 256 values, tile t = [256 t,
// min(n, 256 t + 256)); lane t of the block's one wave owns tile t and adds its terms in index order; the 64 lanes' partials (+0.0 for a lane
// without a tile) are folded by the xor butterfly, which is the fixed pairwise tree over the tile index that k_fig_fold walks.  No
// floating-point atomics, no other cross-lane sum: a fit is a function of its segment's values alone, whatever the grid and the batch.
// A block is therefore one wave (LQ_MIX_THREADS = 64): more lanes would have no tile to own.  The batch is what fills the device.
//
// WHERE THE DATA LIVE.  A lane walks 256 values, too many for its registers, so the segment lies in LDS for all iterations, transposed
// (value i of tile t at [i * LQ_MIX_MAX_TILES + t]: the lanes of a step read neighbouring doubles, no bank conflict); k_mix_lognorm keeps
// log(x), computed once, beside it.  LQ_MIX_MAX_N is 9216 = 36 tiles and not 16384: two arrays of 16384 doubles are 256 KiB, a CU has 160 KiB;
// 2 x 72 KiB fit (one block per CU for k_mix_lognorm, two for k_mix_gmm2 with its one array), and 9216 covers what LongQC can ask for: at
// most 10000 sampled reads, of which the fits see the values below the 85 % quantile.  The responsibilities are not stored (a third and
// fourth array would not fit): the pass that needs the new means for the variances computes the E-step again from the old parameters.
//
// NO FUSED ARITHMETIC, as in kernels_boxstats.hpp: every double operation goes through LQ_MIX_MUL / ADD / SUB / DIV / SQRT (the __d*_rn
// intrinsics, which never fuse; plain operators in the emulator build), so that the emulator and the device differ in exp and log alone.
#pragma once
#include "lq_common.hpp"
#include <cmath>

#define LQ_MIX_THREADS 64
#define LQ_MIX_TILE 256u
#define LQ_MIX_MAX_TILES 36u
#define LQ_MIX_MAX_N 9216u           // LQ_MIX_TILE * LQ_MIX_MAX_TILES (mixfit.cpp asserts it)
#define LQ_MIX_MAX_BLOCKS 1024u      // fits of one round of a launch; the others go round again
#define LQ_MIX_MAX_TOL_ITERS 64u     // mixem's tol_iters: the log-likelihoods kept for its stopping rule
#define LQ_MIX_EXIT_TOL 0u
#define LQ_MIX_EXIT_MAX 1u
#define LQ_MIX_EXIT_NAN 2u
#define LQ_MIX_LOG_2PI 1.8378770664093453        // np.log(2 * np.pi)
#define LQ_MIX_HALF_LOG_2PI 0.9189385332046727   // 0.5 * np.log(2 * np.pi)
#define LQ_MIX_TEN_EPS 2.220446049250313e-15     // 10 * np.finfo(np.float64).eps

#ifndef LQ_EMU
#define LQ_MIX_MUL(a, b) __dmul_rn((a), (b))
#define LQ_MIX_ADD(a, b) __dadd_rn((a), (b))
#define LQ_MIX_SUB(a, b) __dsub_rn((a), (b))
#define LQ_MIX_DIV(a, b) __ddiv_rn((a), (b))
#define LQ_MIX_SQRT(a) __dsqrt_rn(a)
#else
#define LQ_MIX_MUL(a, b) ((a) * (b))
#define LQ_MIX_ADD(a, b) ((a) + (b))
#define LQ_MIX_SUB(a, b) ((a) - (b))
#define LQ_MIX_DIV(a, b) ((a) / (b))
#define LQ_MIX_SQRT(a) sqrt(a)
#endif

// lqmix_fit of include/lqcov.h, field for field (mixfit.cpp asserts the size)
struct LqMixFit {
	double w[2], mu[2], s[2];        // s: the variances (k_mix_gmm2) or the sigmas (k_mix_lognorm)
	double ll;
	u32 n_iter, exit;
	u64 n;
};

// the tiles' partials folded over the lane index: lanes (2 o) q and (2 o) q + o, a pairwise tree (every lane gets the sum: a + b == b + a)
__device__ __forceinline__ double lq_mix_fold(double s)
{
	for (int o = 1; o < 64; o <<= 1) s = LQ_MIX_ADD(s, __shfl_xor(s, o));
	return s;
}

// segment -> LDS, transposed; lx: log(x) beside it (or null)
__device__ __forceinline__ void lq_mix_load(const double *x, u32 n, double *s_x, double *s_lx)
{
	for (u32 g = threadIdx.x; g < n; g += LQ_MIX_THREADS) {
		const u32 at = (g % LQ_MIX_TILE) * LQ_MIX_MAX_TILES + g / LQ_MIX_TILE;
		const double v = x[g];
		s_x[at] = v;
		if (s_lx) s_lx[at] = log(v);
	}
}

// The first pass of an iteration: out = { sum r0, sum r1, sum r0 d0, sum r1 d1, sum extra }, d0 = x, d1 = s_d1's value (x again for two
// Gaussians, log x for the log-normal).  resp(index, x, d1, r0, r1, extra): the E-step of one value from the parameters in force.
template <class R> __device__ __forceinline__ void lq_mix_pass_sums(const double *s_x, const double *s_d1, u32 n, R resp, double *out)
{
	const u32 t = threadIdx.x, first = t * LQ_MIX_TILE;
	const u32 cnt = first >= n ? 0 : n - first < LQ_MIX_TILE ? n - first : LQ_MIX_TILE;
	double a0 = 0.0, a1 = 0.0, b0 = 0.0, b1 = 0.0, c = 0.0;
	for (u32 i = 0; i < cnt; ++i) {
		const double x = s_x[i * LQ_MIX_MAX_TILES + t], d1 = s_d1[i * LQ_MIX_MAX_TILES + t];
		double r0, r1, e;
		resp(first + i, x, d1, r0, r1, e);
		a0 = LQ_MIX_ADD(a0, r0); a1 = LQ_MIX_ADD(a1, r1);
		b0 = LQ_MIX_ADD(b0, LQ_MIX_MUL(r0, x)); b1 = LQ_MIX_ADD(b1, LQ_MIX_MUL(r1, d1));
		c = LQ_MIX_ADD(c, e);
	}
	out[0] = lq_mix_fold(a0); out[1] = lq_mix_fold(a1); out[2] = lq_mix_fold(b0); out[3] = lq_mix_fold(b1); out[4] = lq_mix_fold(c);
}

// The second pass: out = { sum r0 (d0 - m0)^2, sum r1 (d1 - m1)^2 } with the responsibilities of the same parameters as the first pass.
// SKL: sklearn's (r * diff) * diff; otherwise mixem's r * (diff * diff).
template <bool SKL, class R> __device__ __forceinline__ void lq_mix_pass_sq(const double *s_x, const double *s_d1, u32 n, R resp, double m0, double m1, double *out)
{
	const u32 t = threadIdx.x, first = t * LQ_MIX_TILE;
	const u32 cnt = first >= n ? 0 : n - first < LQ_MIX_TILE ? n - first : LQ_MIX_TILE;
	double e0 = 0.0, e1 = 0.0;
	for (u32 i = 0; i < cnt; ++i) {
		const double x = s_x[i * LQ_MIX_MAX_TILES + t], d1 = s_d1[i * LQ_MIX_MAX_TILES + t];
		double r0, r1, e;
		resp(first + i, x, d1, r0, r1, e);
		const double u0 = LQ_MIX_SUB(x, m0), u1 = LQ_MIX_SUB(d1, m1);
		if (SKL) { e0 = LQ_MIX_ADD(e0, LQ_MIX_MUL(LQ_MIX_MUL(r0, u0), u0)); e1 = LQ_MIX_ADD(e1, LQ_MIX_MUL(LQ_MIX_MUL(r1, u1), u1)); }
		else { e0 = LQ_MIX_ADD(e0, LQ_MIX_MUL(r0, LQ_MIX_MUL(u0, u0))); e1 = LQ_MIX_ADD(e1, LQ_MIX_MUL(r1, LQ_MIX_MUL(u1, u1))); }
	}
	out[0] = lq_mix_fold(e0); out[1] = lq_mix_fold(e1);
}

// ---- two Gaussians, as sklearn fits them -----------------------------------------------------------------------------------------------
struct LqGmmPar {
	double w[2], mu[2], var[2];
	double pc[2], mp[2], ld[2], lw[2];       // the precision's square root (1 / sqrt(var)), mu * pc, log(pc), log(w)
};

__device__ __forceinline__ void lq_gmm_derive(LqGmmPar &p)
{
	for (int k = 0; k < 2; ++k) {
		p.pc[k] = LQ_MIX_DIV(1.0, LQ_MIX_SQRT(p.var[k]));
		p.mp[k] = LQ_MIX_MUL(p.mu[k], p.pc[k]);
		p.ld[k] = log(p.pc[k]);
		p.lw[k] = log(p.w[k]);
	}
}

// _estimate_log_gaussian_prob + log weights, logsumexp, exp(log_resp); e = the value's normalised log-probability
struct LqGmmResp {
	LqGmmPar p;
	__device__ __forceinline__ void operator()(u32, double x, double, double &r0, double &r1, double &e) const
	{
		const double y0 = LQ_MIX_SUB(LQ_MIX_MUL(x, p.pc[0]), p.mp[0]), y1 = LQ_MIX_SUB(LQ_MIX_MUL(x, p.pc[1]), p.mp[1]);
		const double l0 = LQ_MIX_ADD(LQ_MIX_ADD(LQ_MIX_MUL(-0.5, LQ_MIX_ADD(LQ_MIX_LOG_2PI, LQ_MIX_MUL(y0, y0))), p.ld[0]), p.lw[0]);
		const double l1 = LQ_MIX_ADD(LQ_MIX_ADD(LQ_MIX_MUL(-0.5, LQ_MIX_ADD(LQ_MIX_LOG_2PI, LQ_MIX_MUL(y1, y1))), p.ld[1]), p.lw[1]);
		const double m = l0 > l1 ? l0 : l1;
		e = LQ_MIX_ADD(m, log(LQ_MIX_ADD(exp(LQ_MIX_SUB(l0, m)), exp(LQ_MIX_SUB(l1, m)))));
		r0 = exp(LQ_MIX_SUB(l0, e)); r1 = exp(LQ_MIX_SUB(l1, e));
	}
};

// the initialisation's responsibilities: one-hot, the first `split` values are component 0
struct LqSplitResp {
	u32 split;
	__device__ __forceinline__ void operator()(u32 g, double, double, double &r0, double &r1, double &e) const
	{
		r0 = g < split ? 1.0 : 0.0; r1 = g < split ? 0.0 : 1.0; e = 0.0;
	}
};

// _estimate_gaussian_parameters from the two passes' sums; the weights are nk (the caller normalises them its way)
template <class R> __device__ __forceinline__ double lq_gmm_mstep(const double *s_x, u32 n, R resp, double reg_covar, LqGmmPar &q)
{
	double s[5], e[2];
	lq_mix_pass_sums(s_x, s_x, n, resp, s);
	q.w[0] = LQ_MIX_ADD(s[0], LQ_MIX_TEN_EPS); q.w[1] = LQ_MIX_ADD(s[1], LQ_MIX_TEN_EPS);
	q.mu[0] = LQ_MIX_DIV(s[2], q.w[0]); q.mu[1] = LQ_MIX_DIV(s[3], q.w[1]);
	lq_mix_pass_sq<true>(s_x, s_x, n, resp, q.mu[0], q.mu[1], e);
	q.var[0] = LQ_MIX_ADD(LQ_MIX_DIV(e[0], q.w[0]), reg_covar); q.var[1] = LQ_MIX_ADD(LQ_MIX_DIV(e[1], q.w[1]), reg_covar);
	return s[4];
}

// x: the fits' segments, each ascending; off[f] .. off[f + 1]: segment f; split[f]: its start.  The components come out ascending in mean.
__global__ void __launch_bounds__(LQ_MIX_THREADS)
k_mix_gmm2(const double *x, const u64 *off, const u32 *split, u32 n_fits, double tol, u32 max_iter, double reg_covar, LqMixFit *out)
{
	__shared__ double s_x[LQ_MIX_MAX_N];
	for (u32 f = blockIdx.x; f < n_fits; f += gridDim.x) {
		const u32 n = (u32)(off[f + 1] - off[f]);
		__syncthreads();                                        // (the last fit's reads are over)
		lq_mix_load(x + off[f], n, s_x, nullptr);
		__syncthreads();
		LqGmmResp cur;
		LqSplitResp start;
		start.split = split[f];
		lq_gmm_mstep(s_x, n, start, reg_covar, cur.p);
		cur.p.w[0] = LQ_MIX_DIV(cur.p.w[0], (double)n); cur.p.w[1] = LQ_MIX_DIV(cur.p.w[1], (double)n);      // _initialize: weights /= n_samples
		lq_gmm_derive(cur.p);
		double bound = -INFINITY;
		u32 it = 0, exit = LQ_MIX_EXIT_MAX;
		while (it < max_iter) {
			++it;
			const double prev = bound;
			LqGmmPar q;
			bound = LQ_MIX_DIV(lq_gmm_mstep(s_x, n, cur, reg_covar, q), (double)n);
			const double wsum = LQ_MIX_ADD(q.w[0], q.w[1]);                    // _m_step: weights_ /= weights_.sum()
			q.w[0] = LQ_MIX_DIV(q.w[0], wsum); q.w[1] = LQ_MIX_DIV(q.w[1], wsum);
			cur.p = q;
			lq_gmm_derive(cur.p);
			if (fabs(LQ_MIX_SUB(bound, prev)) < tol) { exit = LQ_MIX_EXIT_TOL; break; }
		}
		if (threadIdx.x == 0) {
			const int a = cur.p.mu[1] < cur.p.mu[0] ? 1 : 0, b = a ^ 1;
			LqMixFit r;
			r.w[0] = cur.p.w[a]; r.w[1] = cur.p.w[b]; r.mu[0] = cur.p.mu[a]; r.mu[1] = cur.p.mu[b]; r.s[0] = cur.p.var[a]; r.s[1] = cur.p.var[b];
			r.ll = bound; r.n_iter = it; r.exit = exit; r.n = n;
			out[f] = r;
		}
	}
}

// ---- a normal and a log-normal, as mixem fits them -------------------------------------------------------------------------------------
struct LqLognResp {
	double w[2], mu[2], sg[2];
	double den[2], ls[2];                     // 2 sigma^2, log(sigma)
	__device__ __forceinline__ void derive()
	{
		for (int k = 0; k < 2; ++k) { den[k] = LQ_MIX_MUL(2.0, LQ_MIX_MUL(sg[k], sg[k])); ls[k] = log(sg[k]); }
	}
	// log_density of both, resp = w exp(log_density) normalised; e = the value's share of sum(resp * log_density)
	__device__ __forceinline__ void operator()(u32, double x, double lx, double &r0, double &r1, double &e) const
	{
		const double u0 = LQ_MIX_SUB(x, mu[0]), u1 = LQ_MIX_SUB(lx, mu[1]);
		const double l0 = LQ_MIX_SUB(LQ_MIX_SUB(LQ_MIX_DIV(-LQ_MIX_MUL(u0, u0), den[0]), ls[0]), LQ_MIX_HALF_LOG_2PI);
		const double l1 = LQ_MIX_SUB(LQ_MIX_SUB(LQ_MIX_SUB(LQ_MIX_DIV(-LQ_MIX_MUL(u1, u1), den[1]), ls[1]), LQ_MIX_HALF_LOG_2PI), lx);
		const double p0 = LQ_MIX_MUL(w[0], exp(l0)), p1 = LQ_MIX_MUL(w[1], exp(l1)), tot = LQ_MIX_ADD(p0, p1);
		r0 = LQ_MIX_DIV(p0, tot); r1 = LQ_MIX_DIV(p1, tot);
		e = LQ_MIX_ADD(LQ_MIX_MUL(r0, l0), LQ_MIX_MUL(r1, l1));
	}
};

// init[4 f ..]: mu and sigma of the normal, mu and sigma of the log-normal.  Component 0 is the normal, 1 the log-normal.
__global__ void __launch_bounds__(LQ_MIX_THREADS)
k_mix_lognorm(const double *x, const u64 *off, const double *init, u32 n_fits, double tol, u32 tol_iters, u32 max_iter, LqMixFit *out)
{
	__shared__ double s_x[LQ_MIX_MAX_N];
	__shared__ double s_lx[LQ_MIX_MAX_N];
	__shared__ double s_ll[LQ_MIX_MAX_TOL_ITERS];               // last_ll as a ring: every lane writes the same value and reads its own
	for (u32 f = blockIdx.x; f < n_fits; f += gridDim.x) {
		const u32 n = (u32)(off[f + 1] - off[f]);
		__syncthreads();
		lq_mix_load(x + off[f], n, s_x, s_lx);
		__syncthreads();
		LqLognResp cur;
		cur.w[0] = cur.w[1] = 1.0;
		cur.mu[0] = init[4 * f]; cur.sg[0] = init[4 * f + 1]; cur.mu[1] = init[4 * f + 2]; cur.sg[1] = init[4 * f + 3];
		cur.derive();
		for (u32 k = 0; k < tol_iters; ++k) s_ll[k] = 0.0;
		double ll = 0.0;
		u32 it = 0, exit;
		for (;;) {
			double s[5], e[2];
			lq_mix_pass_sums(s_x, s_lx, n, cur, s);
			ll = s[4];
			const double m0 = LQ_MIX_DIV(s[2], s[0]), m1 = LQ_MIX_DIV(s[3], s[1]);
			lq_mix_pass_sq<false>(s_x, s_lx, n, cur, m0, m1, e);
			cur.mu[0] = m0; cur.mu[1] = m1;
			cur.sg[0] = LQ_MIX_SQRT(LQ_MIX_DIV(e[0], s[0])); cur.sg[1] = LQ_MIX_SQRT(LQ_MIX_DIV(e[1], s[1]));
			cur.w[0] = LQ_MIX_DIV(s[0], (double)n); cur.w[1] = LQ_MIX_DIV(s[1], (double)n);
			cur.derive();
			if (ll != ll) { exit = LQ_MIX_EXIT_NAN; break; }
			const double back = s_ll[it % tol_iters];                 // from iteration tol_iters on: the value of tol_iters iterations ago
			if (it >= tol_iters && LQ_MIX_DIV(LQ_MIX_SUB(back, ll), back) <= tol) { exit = LQ_MIX_EXIT_TOL; break; }
			if (it >= max_iter) { exit = LQ_MIX_EXIT_MAX; break; }
			__syncthreads();                                          // (every lane has read the slot before any lane overwrites it; ll is the same in all)
			s_ll[it % tol_iters] = ll;
			++it;
		}
		if (threadIdx.x == 0) {
			LqMixFit r;
			r.w[0] = cur.w[0]; r.w[1] = cur.w[1]; r.mu[0] = cur.mu[0]; r.mu[1] = cur.mu[1]; r.s[0] = cur.sg[0]; r.s[1] = cur.sg[1];
			r.ll = ll; r.n_iter = it + 1; r.exit = exit; r.n = n;
			out[f] = r;
		}
	}
}
