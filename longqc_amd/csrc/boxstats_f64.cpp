// longqc_amd/csrc/boxstats_f64.cpp -- host side of the grouped box-plot statistics over doubles (kernels_boxstats_f64.hpp) behind the C ABI
// of include/lqcov.h: lqfig_boxstats_f64, an array-level call like lqfig_boxstats, and lq_box_f64_dev (boxstats_dev.hpp) for a caller
// whose two arrays lie on the device already (csv.cpp).  boxstats.cpp and its kernels are not touched: kernels_boxstats.hpp is
// included here for its LQ_BOX_* macros and k_box_heads, inside a namespace so that this file's copies of its kernels have names of their own.
#include "lq_cabi.hpp"
#include "boxstats_dev.hpp"
#include <cmath>
#include <cstdlib>

namespace lq_box_thou {
#include "kernels_boxstats.hpp"
}
using lq_box_thou::k_box_heads;
#include "kernels_boxstats_f64.hpp"

namespace {
static_assert(sizeof(LqBoxD) == sizeof(lqfig_box_f64) && sizeof(lqfig_box_f64) == 104, "LqBoxD is lqfig_box_f64");

// blocks of a launch: LQ_BOX_MAX_BLOCKS, or fewer with LQBOX_TEST_MAX_BLOCKS (boxstats.cpp's test hook: the results may not change with it)
u32 max_blocks()
{
	const char *v = getenv("LQBOX_TEST_MAX_BLOCKS");
	const long n = v ? atol(v) : 0;
	return n > 0 && (u64)n < LQ_BOX_MAX_BLOCKS ? (u32)n : LQ_BOX_MAX_BLOCKS;
}

u32 grid_for(u64 items)
{
	const u64 g = (items + LQ_BOX_THREADS - 1) / LQ_BOX_THREADS, cap = max_blocks();
	return (u32)(g < 1 ? 1 : g > cap ? cap : g);
}
} // namespace

void lq_box_f64_dev(hipStream_t s, const u32 *d_key, const double *d_x, u64 n, double interval, double whis, double *sorted, lqfig_box_f64 *boxes,
                    u32 box_cap, u32 *n_boxes)
{
	*n_boxes = 0;
	if (!std::isfinite(interval) || interval < 0) throw std::invalid_argument("the interval is not a finite number of 0 or more");
	if (!std::isfinite(whis) || whis < 0) throw std::invalid_argument("whis is not a finite number of 0 or more");
	if (n >= (1ULL << 32)) throw std::domain_error("an array of 2^32 values or more");
	if (n == 0) return;
	if (!sorted || (box_cap && !boxes)) throw std::invalid_argument("null buffers");
	DBuf vk, vks, idx0, idx1, idx2, grp, g2, gs, ctl, d_sorted, flag, pos, head, d_box;
	Prim prim;
	prim.stream = s;
	vk.ensure((size_t)n * 8); vks.ensure((size_t)n * 8); idx0.ensure((size_t)n * 8); idx1.ensure((size_t)n * 8); idx2.ensure((size_t)n * 8);
	grp.ensure((size_t)n * 4); g2.ensure((size_t)n * 4); gs.ensure((size_t)n * 4); ctl.ensure(8);
	LQ_HIP_CHECK(hipMemsetAsync(ctl.p, 0, 8, s));
	LQ_LAUNCH(k_boxd_keys, grid_for(n), LQ_BOX_THREADS, s, d_key, d_x, n, interval, vk.as<u64>(), idx0.as<u64>(), grp.as<u32>(), ctl.as<u32>());
	LQ_HIP_CHECK(hipGetLastError());
	u32 c[2];
	LQ_HIP_CHECK(hipMemcpyAsync(c, ctl.p, 8, hipMemcpyDeviceToHost, s));
	LQ_HIP_CHECK(hipStreamSynchronize(s));
	if (c[1] & 2u) throw std::domain_error("a group of 2^32 or more");
	if (c[1] & 1u) throw std::domain_error("a value that is NaN: it has no place in the order");
	u32 gbits = 1;
	while (gbits < 32 && (c[0] >> gbits)) ++gbits;
	prim.radix<u64, u64, true>(vk.as<u64>(), vks.as<u64>(), idx0.as<u64>(), idx1.as<u64>(), (size_t)n, 64);
	LQ_LAUNCH(k_boxd_rekey, grid_for(n), LQ_BOX_THREADS, s, (const u32*)grp.as<u32>(), (const u64*)idx1.as<u64>(), n, g2.as<u32>());
	prim.radix<u32, u64, true>(g2.as<u32>(), gs.as<u32>(), idx1.as<u64>(), idx2.as<u64>(), (size_t)n, gbits);
	d_sorted.ensure((size_t)n * 8); flag.ensure(((size_t)n + 1) * 4); pos.ensure(((size_t)n + 1) * 4);
	LQ_LAUNCH(k_boxd_flags, grid_for(n + 1), LQ_BOX_THREADS, s, (const u32*)gs.as<u32>(), (const u64*)idx2.as<u64>(), d_x, n, d_sorted.as<double>(), flag.as<u32>());
	LQ_HIP_CHECK(hipGetLastError());
	prim.exclusive_scan_u32_u32(flag.as<u32>(), pos.as<u32>(), (size_t)n + 1);
	u32 groups = 0;
	LQ_HIP_CHECK(hipMemcpyAsync(&groups, pos.as<u32>() + n, 4, hipMemcpyDeviceToHost, s));
	LQ_HIP_CHECK(hipStreamSynchronize(s));
	if (groups < 1 || groups > n) throw std::logic_error("the groups' heads do not fit the array");
	*n_boxes = groups;
	if (groups > box_cap) throw std::invalid_argument("box_cap is smaller than the number of groups");
	head.ensure(((size_t)groups + 1) * 4); d_box.ensure((size_t)groups * sizeof(LqBoxD));
	LQ_LAUNCH(k_box_heads, grid_for(n), LQ_BOX_THREADS, s, flag.as<u32>(), pos.as<u32>(), n, head.as<u32>());
	LQ_LAUNCH(k_boxd_stats, grid_for(groups), LQ_BOX_THREADS, s, (const u32*)gs.as<u32>(), (const double*)d_sorted.as<double>(), (const u32*)head.as<u32>(), groups, whis, d_box.as<LqBoxD>());
	LQ_HIP_CHECK(hipGetLastError());
	LQ_HIP_CHECK(hipMemcpyAsync(sorted, d_sorted.p, (size_t)n * 8, hipMemcpyDeviceToHost, s));
	LQ_HIP_CHECK(hipMemcpyAsync(boxes, d_box.p, (size_t)groups * sizeof(LqBoxD), hipMemcpyDeviceToHost, s));
	LQ_HIP_CHECK(hipStreamSynchronize(s));
}

extern "C" {

int lqfig_boxstats_f64(int device, const uint32_t *key, const double *x, uint64_t n, double interval, double whis,
                       double *sorted, lqfig_box_f64 *boxes, uint32_t box_cap, uint32_t *n_boxes, char *errbuf, size_t errbuf_len)
{
	return lq_cabi::guarded(errbuf, errbuf_len, [&] {
		if (!n_boxes) throw std::invalid_argument("null buffers");
		*n_boxes = 0;
		if (n >= (1ULL << 32)) throw std::domain_error("an array of 2^32 values or more");
		if (n && (!key || !x)) throw std::invalid_argument("null buffers");
		lq_cabi::ScopedStream s(device);
		DBuf d_key, d_x;
		try {
			if (n) {
				d_key.ensure((size_t)n * 4); d_x.ensure((size_t)n * 8);
				LQ_HIP_CHECK(hipMemcpyAsync(d_key.p, key, (size_t)n * 4, hipMemcpyHostToDevice, s));
				LQ_HIP_CHECK(hipMemcpyAsync(d_x.p, x, (size_t)n * 8, hipMemcpyHostToDevice, s));
			}
			lq_box_f64_dev(s, d_key.as<u32>(), d_x.as<double>(), n, interval, whis, sorted, boxes, box_cap, n_boxes);
		} catch (...) { (void)hipStreamSynchronize(s); throw; }      // (the copies read and write the caller's arrays: none stays queued)
	});
}

} // extern "C"
