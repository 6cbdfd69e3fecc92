// longqc_amd/csrc/mixfit.cpp -- host side of the two mixture fits (kernels_mixfit.hpp) behind the C ABI of include/lqcov.h: lqmix_gmm2,
// lqmix_lognorm.  Array-level calls like the lqfig_* calls (figdata.cpp): each sorts its segments, uploads them, runs one launch on a stream
// of its own and brings back one lqmix_fit per segment; nothing stays resident.  The start of the Gaussian fit is found here, in plain
// sequential double: the split of the sorted values with the smallest two-cluster squared error.
#include "lq_cabi.hpp"
#include "kernels_mixfit.hpp"
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <vector>

namespace {
static_assert(sizeof(LqMixFit) == sizeof(lqmix_fit) && sizeof(lqmix_fit) == 72, "LqMixFit is lqmix_fit");
static_assert(LQ_MIX_MAX_N == LQMIX_MAX_N && LQ_MIX_TILE * LQ_MIX_MAX_TILES == LQ_MIX_MAX_N, "the largest segment");
static_assert(LQ_MIX_MAX_TILES <= LQ_MIX_THREADS, "a lane per tile");
static_assert(LQ_MIX_EXIT_TOL == LQMIX_EXIT_TOL && LQ_MIX_EXIT_MAX == LQMIX_EXIT_MAX && LQ_MIX_EXIT_NAN == LQMIX_EXIT_NAN, "the exits");

// blocks of a launch: LQ_MIX_MAX_BLOCKS, or fewer with LQMIX_TEST_MAX_BLOCKS (a test hook: the results may not change with it)
u32 grid_for(u32 n_fits)
{
	const char *v = getenv("LQMIX_TEST_MAX_BLOCKS");
	const long n = v ? atol(v) : 0;
	const u32 cap = n > 0 && (u64)n < LQ_MIX_MAX_BLOCKS ? (u32)n : LQ_MIX_MAX_BLOCKS;
	return n_fits < cap ? n_fits : cap;
}

// the segments checked and sorted ascending, one after the other from 0 on -> (values, offsets)
void sorted_segments(const double *x, const u64 *off, u32 n_fits, bool positive, std::vector<double> &xs, std::vector<u64> &offs)
{
	if (!x || !off) throw std::invalid_argument("null buffers");
	if (n_fits == 0) throw std::invalid_argument("no fits");
	offs.assign((size_t)n_fits + 1, 0);
	for (u32 f = 0; f < n_fits; ++f) {
		if (off[f + 1] < off[f]) throw std::invalid_argument("offsets are not ascending");
		const u64 n = off[f + 1] - off[f];
		if (n < 2) throw std::invalid_argument("a segment of fewer than 2 values");
		if (n > LQ_MIX_MAX_N) throw std::invalid_argument("a segment of more than LQMIX_MAX_N values");
		offs[f + 1] = offs[f] + n;
	}
	xs.resize((size_t)offs[n_fits]);
	for (u32 f = 0; f < n_fits; ++f) {
		double *s = xs.data() + offs[f];
		const size_t n = (size_t)(offs[f + 1] - offs[f]);
		for (size_t i = 0; i < n; ++i) {
			const double v = x[off[f] + i];
			if (!std::isfinite(v)) throw std::invalid_argument("a value that is not finite");
			if (positive && !(v > 0)) throw std::invalid_argument("a value that is not positive has no logarithm");
			s[i] = v == 0 ? 0.0 : v;                              // (-0.0 sorts and adds like 0.0: one representation)
		}
		std::sort(s, s + n);
		if (s[0] == s[n - 1]) throw std::invalid_argument("a segment without variance: all its values are equal");
	}
}

// the smallest k in [1, n - 1] at the minimum of the squared error of {s[0 .. k)} + {s[k .. n)}, from running sums of x and x * x
u32 best_split(const double *s, size_t n)
{
	double t1 = 0.0, t2 = 0.0;
	for (size_t i = 0; i < n; ++i) { t1 += s[i]; t2 += s[i] * s[i]; }
	double a1 = 0.0, a2 = 0.0, best = INFINITY;
	u32 best_k = 1;
	for (size_t k = 1; k < n; ++k) {
		a1 += s[k - 1]; a2 += s[k - 1] * s[k - 1];
		const double b1 = t1 - a1, b2 = t2 - a2;
		const double sse = (a2 - a1 * a1 / (double)k) + (b2 - b1 * b1 / (double)(n - k));
		if (sse < best) { best = sse; best_k = (u32)k; }
	}
	return best_k;
}

void upload(DBuf &b, const void *src, size_t bytes, hipStream_t s)
{
	b.ensure(bytes);
	LQ_HIP_CHECK(hipMemcpyAsync(b.p, src, bytes, hipMemcpyHostToDevice, s));
}
} // namespace

extern "C" {

int lqmix_gmm2(int device, const double *x, const uint64_t *off, uint32_t n_fits, double tol, uint32_t max_iter, double reg_covar,
               lqmix_fit *out, char *errbuf, size_t errbuf_len)
{
	return lq_cabi::guarded(errbuf, errbuf_len, [&] {
		if (!out) throw std::invalid_argument("null buffers");
		if (std::isnan(tol)) throw std::invalid_argument("tol is NaN");
		if (max_iter == 0) throw std::invalid_argument("max_iter is 0");
		if (!std::isfinite(reg_covar) || reg_covar < 0) throw std::invalid_argument("reg_covar is not a finite number of 0 or more");
		std::vector<double> xs;
		std::vector<u64> offs;
		const double t0 = lq_now_s();
		sorted_segments(x, off, n_fits, false, xs, offs);
		std::vector<u32> split(n_fits);
		for (u32 f = 0; f < n_fits; ++f) split[f] = best_split(xs.data() + offs[f], (size_t)(offs[f + 1] - offs[f]));
		const double t1 = lq_now_s();
		lq_cabi::ScopedStream s(device);
		DBuf d_x, d_off, d_split, d_out;
		upload(d_x, xs.data(), xs.size() * 8, s);
		upload(d_off, offs.data(), offs.size() * 8, s);
		upload(d_split, split.data(), split.size() * 4, s);
		d_out.ensure((size_t)n_fits * sizeof(LqMixFit));
		LQ_LAUNCH(k_mix_gmm2, grid_for(n_fits), LQ_MIX_THREADS, s, d_x.as<double>(), d_off.as<u64>(), d_split.as<u32>(), (u32)n_fits, tol, (u32)max_iter,
		          reg_covar, d_out.as<LqMixFit>());
		LQ_HIP_CHECK(hipGetLastError());
		LQ_HIP_CHECK(hipMemcpyAsync(out, d_out.p, (size_t)n_fits * sizeof(LqMixFit), hipMemcpyDeviceToHost, s));
		LQ_HIP_CHECK(hipStreamSynchronize(s));
		if (getenv("LQCOV_TIMING"))                                 // the call's two halves on stderr: the host's sorts and split searches, then stream, upload, launch and read-back
			fprintf(stderr, "lqmix_gmm2: fits %u values %llu: sort + split %.3f device %.3f ms\n", n_fits, (unsigned long long)xs.size(), (t1 - t0) * 1e3, (lq_now_s() - t1) * 1e3);
	});
}

int lqmix_lognorm(int device, const double *x, const uint64_t *off, uint32_t n_fits, const double *init, double tol, uint32_t tol_iters,
                  uint32_t max_iter, lqmix_fit *out, char *errbuf, size_t errbuf_len)
{
	return lq_cabi::guarded(errbuf, errbuf_len, [&] {
		if (!out || !init) throw std::invalid_argument("null buffers");
		if (std::isnan(tol)) throw std::invalid_argument("tol is NaN");
		if (tol_iters < 1 || tol_iters > LQ_MIX_MAX_TOL_ITERS) throw std::invalid_argument("tol_iters is outside [1, 64]");
		std::vector<double> xs;
		std::vector<u64> offs;
		sorted_segments(x, off, n_fits, true, xs, offs);
		for (u32 f = 0; f < n_fits; ++f) {
			const double *p = init + 4 * (size_t)f;
			if (!std::isfinite(p[0]) || !std::isfinite(p[2])) throw std::invalid_argument("a starting mu that is not finite");
			if (!std::isfinite(p[1]) || !std::isfinite(p[3]) || !(p[1] > 0) || !(p[3] > 0)) throw std::invalid_argument("a starting sigma that is not positive and finite");
		}
		lq_cabi::ScopedStream s(device);
		DBuf d_x, d_off, d_init, d_out;
		upload(d_x, xs.data(), xs.size() * 8, s);
		upload(d_off, offs.data(), offs.size() * 8, s);
		upload(d_init, init, (size_t)n_fits * 32, s);
		d_out.ensure((size_t)n_fits * sizeof(LqMixFit));
		LQ_LAUNCH(k_mix_lognorm, grid_for(n_fits), LQ_MIX_THREADS, s, d_x.as<double>(), d_off.as<u64>(), d_init.as<double>(), (u32)n_fits, tol, (u32)tol_iters,
		          (u32)max_iter, d_out.as<LqMixFit>());
		LQ_HIP_CHECK(hipGetLastError());
		LQ_HIP_CHECK(hipMemcpyAsync(out, d_out.p, (size_t)n_fits * sizeof(LqMixFit), hipMemcpyDeviceToHost, s));
		LQ_HIP_CHECK(hipStreamSynchronize(s));
	});
}

} // extern "C"
