// longqc_amd/csrc/figdata.cpp -- host side of the figure data (kernels_figdata.hpp) behind the C ABI of include/lqcov.h: lqfig_range,
// lqfig_hist, lqfig_kde, lqfig_logsum.  Array-level calls in the style of lqgc_reads: each uploads its array, runs on a stream of its own
// and brings back a few numbers; nothing stays resident.  The tiles of the two floating-point sums and the tree that folds them depend
// on n alone; the grid only decides which wave takes which tile.
#include "lq_cabi.hpp"
#include "kernels_figdata.hpp"
#include "figdata_dev.hpp"
#include <cmath>
#include <cstdlib>
#include <vector>

namespace {
// blocks of a launch: LQ_FIG_MAX_BLOCKS, or fewer with LQFIG_TEST_MAX_BLOCKS (a test hook: the results may not change with it)
u32 max_blocks()
{
	const char *v = getenv("LQFIG_TEST_MAX_BLOCKS");
	const long n = v ? atol(v) : 0;
	return n > 0 && (u64)n < LQ_FIG_MAX_BLOCKS ? (u32)n : LQ_FIG_MAX_BLOCKS;
}

u32 grid_for(u64 items, u64 per_block)
{
	const u64 g = (items + per_block - 1) / per_block, cap = max_blocks();
	return (u32)(g < 1 ? 1 : g > cap ? cap : g);
}

void check_array(const void *x, u64 n, int dtype)
{
	if (dtype != LQFIG_F32 && dtype != LQFIG_U32) throw std::invalid_argument("dtype is neither LQFIG_F32 nor LQFIG_U32");
	if (n && !x) throw std::invalid_argument("null buffers");
	if (n >= (1ULL << 32)) throw std::domain_error("an array of 2^32 values or more");
}

void upload(DBuf &b, const void *src, size_t bytes, hipStream_t s)
{
	b.ensure(bytes ? bytes : 1);
	if (bytes) LQ_HIP_CHECK(hipMemcpyAsync(b.p, src, bytes, hipMemcpyHostToDevice, s));
}

// part[rows][m] folded over the rows by the fixed tree (k_fig_fold, a level of radix 8 per launch) -> out[m]; rows >= 1
void fold(DBuf &part, u64 rows, u32 m, double *out, hipStream_t s)
{
	DBuf other;
	other.ensure((size_t)((rows + 7) / 8) * m * 8);
	DBuf *in = &part, *to = &other;
	while (rows > 1) {
		const u64 n_out = (rows + 7) / 8 * m;
		LQ_LAUNCH(k_fig_fold, grid_for(n_out, LQ_FIG_THREADS), LQ_FIG_THREADS, s, in->as<double>(), rows, m, to->as<double>());
		LQ_HIP_CHECK(hipGetLastError());
		rows = (rows + 7) / 8;
		std::swap(in, to);
	}
	LQ_HIP_CHECK(hipMemcpyAsync(out, in->p, (size_t)m * 8, hipMemcpyDeviceToHost, s));
	LQ_HIP_CHECK(hipStreamSynchronize(s));
}
} // namespace

// ---- the same two passes over an array that lies on the device already (polread.cpp: the polymerase reads' lengths stay resident) ----
// d_x[0 .. n), n >= 1, n_edges >= 2, the arguments checked by the caller; both wait for the stream
void lq_fig_hist_dev(hipStream_t s, int dtype, const void *d_x, u64 n, const double *edges, u32 n_edges, u64 *counts)
{
	const u32 nb = n_edges - 1;
	DBuf d_e, d_c;
	upload(d_e, edges, (size_t)n_edges * 8, s);
	d_c.ensure((size_t)nb * 8);
	LQ_HIP_CHECK(hipMemsetAsync(d_c.p, 0, (size_t)nb * 8, s));
	const u32 grid = grid_for(n, LQ_FIG_THREADS);
	if (dtype == LQFIG_F32) LQ_LAUNCH(k_fig_hist<float>, grid, LQ_FIG_THREADS, s, (const float*)d_x, (u64)n, d_e.as<double>(), n_edges, d_c.as<unsigned long long>());
	else LQ_LAUNCH(k_fig_hist<u32>, grid, LQ_FIG_THREADS, s, (const u32*)d_x, (u64)n, d_e.as<double>(), n_edges, d_c.as<unsigned long long>());
	LQ_HIP_CHECK(hipGetLastError());
	LQ_HIP_CHECK(hipMemcpyAsync(counts, d_c.p, (size_t)nb * 8, hipMemcpyDeviceToHost, s));
	LQ_HIP_CHECK(hipStreamSynchronize(s));
}

void lq_fig_logsum_dev(hipStream_t s, const u32 *d_x, u64 n, uint64_t *sum, double *sum_log, uint64_t *n_zero)
{
	const u64 n_tiles = (n + LQ_FIG_TILE - 1) / LQ_FIG_TILE;
	DBuf d_tot, d_part;
	d_tot.ensure(16);
	LQ_HIP_CHECK(hipMemsetAsync(d_tot.p, 0, 16, s));
	d_part.ensure((size_t)n_tiles * 8);
	LQ_LAUNCH(k_fig_logsum, grid_for(n_tiles, LQ_FIG_THREADS / 64), LQ_FIG_THREADS, s, d_x, (u64)n, d_tot.as<unsigned long long>(), d_part.as<double>());
	LQ_HIP_CHECK(hipGetLastError());
	unsigned long long tot[2];
	LQ_HIP_CHECK(hipMemcpyAsync(tot, d_tot.p, 16, hipMemcpyDeviceToHost, s));
	fold(d_part, n_tiles, 1, sum_log, s);                     // (waits for the stream)
	*sum = tot[0]; *n_zero = tot[1];
}

extern "C" {

int lqfig_range(int device, int dtype, const void *x, uint64_t n, void *min_out, void *max_out, char *errbuf, size_t errbuf_len)
{
	return lq_cabi::guarded(errbuf, errbuf_len, [&] {
		check_array(x, n, dtype);
		if (!min_out || !max_out) throw std::invalid_argument("null buffers");
		if (n == 0) throw std::invalid_argument("an empty array has no range");
		lq_cabi::ScopedStream s(device);
		DBuf d_x, d_mm;
		upload(d_x, x, (size_t)n * 4, s);
		const u32 init[2] = { 0xffffffffu, 0u };
		u32 mm[2];
		upload(d_mm, init, 8, s);
		LQ_LAUNCH(k_fig_range, grid_for(n, LQ_FIG_THREADS), LQ_FIG_THREADS, s, d_x.as<u32>(), (u64)n, (int)(dtype == LQFIG_F32), d_mm.as<u32>());
		LQ_HIP_CHECK(hipGetLastError());
		LQ_HIP_CHECK(hipMemcpyAsync(mm, d_mm.p, 8, hipMemcpyDeviceToHost, s));
		LQ_HIP_CHECK(hipStreamSynchronize(s));
		if (mm[0] > mm[1]) throw std::invalid_argument("no value that is not NaN");
		if (dtype == LQFIG_F32) { mm[0] = lq_fig_unkey(mm[0]); mm[1] = lq_fig_unkey(mm[1]); }
		memcpy(min_out, mm, 4);
		memcpy(max_out, mm + 1, 4);
	});
}

int lqfig_hist(int device, int dtype, const void *x, uint64_t n, const double *edges, uint32_t n_edges, uint64_t *counts,
               char *errbuf, size_t errbuf_len)
{
	return lq_cabi::guarded(errbuf, errbuf_len, [&] {
		check_array(x, n, dtype);
		if (n_edges && !edges) throw std::invalid_argument("null buffers");
		for (u32 k = 0; k < n_edges; ++k)
			if (std::isnan(edges[k]) || (k && edges[k] < edges[k - 1])) throw std::invalid_argument("edges are not ascending");
		if (n_edges < 2) return;                                  // no bins
		const u32 nb = n_edges - 1;
		if (!counts) throw std::invalid_argument("null buffers");
		for (u32 k = 0; k < nb; ++k) counts[k] = 0;
		if (n == 0) return;
		lq_cabi::ScopedStream s(device);
		DBuf d_x;
		upload(d_x, x, (size_t)n * 4, s);
		lq_fig_hist_dev(s, dtype, d_x.p, n, edges, n_edges, counts);
	});
}

int lqfig_kde(int device, const float *data, uint64_t n, const double *points, uint32_t m, double h, double *sums,
              char *errbuf, size_t errbuf_len)
{
	return lq_cabi::guarded(errbuf, errbuf_len, [&] {
		check_array(data, n, LQFIG_F32);
		if (m == 0) throw std::invalid_argument("no points");
		if (!points || !sums) throw std::invalid_argument("null buffers");
		if (!std::isfinite(h) || h <= 0) throw std::invalid_argument("the bandwidth is not a positive finite number");
		for (u32 j = 0; j < m; ++j) sums[j] = 0.0;
		if (n == 0) return;
		lq_cabi::ScopedStream s(device);
		const u64 n_tiles = (n + LQ_FIG_TILE - 1) / LQ_FIG_TILE;
		DBuf d_x, d_p, d_part;
		upload(d_x, data, (size_t)n * 4, s);
		upload(d_p, points, (size_t)m * 8, s);
		d_part.ensure((size_t)n_tiles * m * 8);
		LQ_LAUNCH(k_fig_kde, grid_for(n_tiles, LQ_FIG_THREADS / 64), LQ_FIG_THREADS, s, d_x.as<float>(), (u64)n, d_p.as<double>(), m, h, d_part.as<double>());
		LQ_HIP_CHECK(hipGetLastError());
		fold(d_part, n_tiles, m, sums, s);
	});
}

int lqfig_logsum(int device, const uint32_t *x, uint64_t n, uint64_t *sum, double *sum_log, uint64_t *n_zero,
                 char *errbuf, size_t errbuf_len)
{
	return lq_cabi::guarded(errbuf, errbuf_len, [&] {
		check_array(x, n, LQFIG_U32);
		if (!sum || !sum_log || !n_zero) throw std::invalid_argument("null buffers");
		*sum = 0; *sum_log = 0.0; *n_zero = 0;
		if (n == 0) return;
		lq_cabi::ScopedStream s(device);
		DBuf d_x;
		upload(d_x, x, (size_t)n * 4, s);
		lq_fig_logsum_dev(s, d_x.as<u32>(), n, sum, sum_log, n_zero);
	});
}

} // extern "C"
