// longqc_amd/csrc/boxstats.cpp -- host side of the grouped box-plot statistics (kernels_boxstats.hpp) behind the C ABI of include/lqcov.h:
// lqfig_boxstats.  An array-level call like the other lqfig_* calls (figdata.cpp): it uploads its two arrays, runs on a stream of its own
// and brings back the sorted values and one lqfig_box per group; nothing stays resident.  The sort is Prim::radix on the keys alone.
#include "lq_cabi.hpp"
#include "kernels_boxstats.hpp"
#include <cmath>
#include <cstdlib>

namespace {
static_assert(sizeof(LqBox) == sizeof(lqfig_box) && sizeof(lqfig_box) == 96, "LqBox is lqfig_box");
static_assert(LQ_BOX_MISSING == LQFIG_MISSING, "the missing value");

// blocks of a launch: LQ_BOX_MAX_BLOCKS, or fewer with LQBOX_TEST_MAX_BLOCKS (a test hook: the results may not change with it)
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

void boxstats_queued(hipStream_t s, const u32 *key, const i32 *thou, u64 n, double interval, double whis, i32 *sorted, lqfig_box *boxes,
                     u32 box_cap, u32 *n_boxes)
{
	DBuf d_key, d_thou, d_k0, d_k1, d_ctl, d_sorted, d_flag, d_pos, d_head, d_box;
	Prim prim;
	prim.stream = s;
	// LQCOV_TIMING: the call's stages on stderr, each closed by a wait for the stream (the waits are the timing's, not the call's)
	const bool timing = getenv("LQCOV_TIMING") != nullptr;
	double t_last = lq_now_s(), t_stage[5] = {0, 0, 0, 0, 0};
	const auto stage = [&](int k, bool wait) {
		if (!timing) return;
		if (wait) LQ_HIP_CHECK(hipStreamSynchronize(s));
		const double now = lq_now_s(); t_stage[k] += now - t_last; t_last = now;
	};
	d_key.ensure((size_t)n * 4); d_thou.ensure((size_t)n * 4); d_k0.ensure((size_t)n * 8); d_k1.ensure((size_t)n * 8); d_ctl.ensure(8);
	stage(0, false);                                            // allocation
	LQ_HIP_CHECK(hipMemcpyAsync(d_key.p, key, (size_t)n * 4, hipMemcpyHostToDevice, s));
	LQ_HIP_CHECK(hipMemcpyAsync(d_thou.p, thou, (size_t)n * 4, hipMemcpyHostToDevice, s));
	LQ_HIP_CHECK(hipMemsetAsync(d_ctl.p, 0, 8, s));
	stage(1, true);                                             // upload
	LQ_LAUNCH(k_box_keys, grid_for(n), LQ_BOX_THREADS, s, d_key.as<u32>(), d_thou.as<i32>(), n, interval, d_k0.as<u64>(), d_ctl.as<u32>());
	LQ_HIP_CHECK(hipGetLastError());
	u32 ctl[2];
	LQ_HIP_CHECK(hipMemcpyAsync(ctl, d_ctl.p, 8, hipMemcpyDeviceToHost, s));
	LQ_HIP_CHECK(hipStreamSynchronize(s));
	if (ctl[1] & 2u) throw std::domain_error("a group of 2^32 or more");
	if (ctl[1] & 1u) throw std::domain_error("a value of INT32_MAX thousandths: its sort key is the missing value's");
	stage(2, false);                                            // keys
	u32 gbits = 0;
	while (gbits < 32 && (ctl[0] >> gbits)) ++gbits;
	prim.radix<u64, u64, false>(d_k0.as<u64>(), d_k1.as<u64>(), nullptr, nullptr, (size_t)n, 32 + gbits, d_k0.as<u64>());
	stage(3, true);                                             // sort
	d_sorted.ensure((size_t)n * 4); d_flag.ensure(((size_t)n + 1) * 4); d_pos.ensure(((size_t)n + 1) * 4);
	LQ_LAUNCH(k_box_flags, grid_for(n + 1), LQ_BOX_THREADS, s, d_k1.as<u64>(), n, d_sorted.as<i32>(), d_flag.as<u32>());
	LQ_HIP_CHECK(hipGetLastError());
	prim.exclusive_scan_u32_u32(d_flag.as<u32>(), d_pos.as<u32>(), (size_t)n + 1);
	u32 groups = 0;
	LQ_HIP_CHECK(hipMemcpyAsync(&groups, d_pos.as<u32>() + n, 4, hipMemcpyDeviceToHost, s));
	LQ_HIP_CHECK(hipStreamSynchronize(s));
	if (groups < 1 || groups > n) throw std::logic_error("the groups' heads do not fit the array");
	*n_boxes = groups;
	if (groups > box_cap) throw std::invalid_argument("box_cap is smaller than the number of groups");
	d_head.ensure(((size_t)groups + 1) * 4); d_box.ensure((size_t)groups * sizeof(LqBox));
	LQ_LAUNCH(k_box_heads, grid_for(n), LQ_BOX_THREADS, s, d_flag.as<u32>(), d_pos.as<u32>(), n, d_head.as<u32>());
	LQ_LAUNCH(k_box_stats, grid_for(groups), LQ_BOX_THREADS, s, d_k1.as<u64>(), d_sorted.as<i32>(), d_head.as<u32>(), groups, whis, d_box.as<LqBox>());
	LQ_HIP_CHECK(hipGetLastError());
	stage(2, true);                                             // heads and statistics (with the keys)
	LQ_HIP_CHECK(hipMemcpyAsync(sorted, d_sorted.p, (size_t)n * 4, hipMemcpyDeviceToHost, s));
	LQ_HIP_CHECK(hipMemcpyAsync(boxes, d_box.p, (size_t)groups * sizeof(LqBox), hipMemcpyDeviceToHost, s));
	LQ_HIP_CHECK(hipStreamSynchronize(s));
	stage(4, false);                                            // download
	if (timing) fprintf(stderr, "lqfig_boxstats: n %llu groups %u: alloc %.3f upload %.3f keys+heads+stats %.3f sort %.3f download %.3f ms\n",
	                    (unsigned long long)n, groups, t_stage[0] * 1e3, t_stage[1] * 1e3, t_stage[2] * 1e3, t_stage[3] * 1e3, t_stage[4] * 1e3);
}
} // namespace

extern "C" {

int lqfig_boxstats(int device, const uint32_t *key, const int32_t *thou, uint64_t n, double interval, double whis,
                   int32_t *sorted, lqfig_box *boxes, uint32_t box_cap, uint32_t *n_boxes, char *errbuf, size_t errbuf_len)
{
	return lq_cabi::guarded(errbuf, errbuf_len, [&] {
		if (!n_boxes) throw std::invalid_argument("null buffers");
		*n_boxes = 0;
		if (!std::isfinite(interval) || interval < 0) throw std::invalid_argument("the interval is not a finite number of 0 or more");
		if (!std::isfinite(whis) || whis < 0) throw std::invalid_argument("whis is not a finite number of 0 or more");
		if (n >= (1ULL << 32)) throw std::domain_error("an array of 2^32 values or more");
		if (n == 0) return;
		if (!key || !thou || !sorted || (box_cap && !boxes)) throw std::invalid_argument("null buffers");
		lq_cabi::ScopedStream s(device);
		try { boxstats_queued(s, key, (const i32*)thou, n, interval, whis, (i32*)sorted, boxes, box_cap, n_boxes); }
		catch (...) { (void)hipStreamSynchronize(s); throw; }        // (the copies read and write the caller's arrays: none stays queued)
	});
}

} // extern "C"
