// longqc_amd/csrc/adapt.cpp -- host side of the adapter search (lq_adapt.py:10-101) behind the C ABI of include/lqcov.h
// (lqadapt_reads).  The host gathers the two end windows of every read of at least 2 * length bases, uploads them in batches,
// runs k_adapt (kernels_adapt.hpp) once per adapter and batch, and scatters the per-end results back to read order.  Which
// reads the reference then skips or trims is decided by the caller (longqc_amd/adapter.py), where lq_adapt.py decides it.
#include "lq_cabi.hpp"
#include "kernels_adapt.hpp"
#include <cstdlib>
#include <vector>

namespace {
struct AdaptDev {
	hipStream_t stream = nullptr;
	DBuf win5, win3, adp5, adp3, out;
	~AdaptDev() { if (stream) { hipStreamSynchronize(stream); hipStreamDestroy(stream); } }
};

// reads per batch: two windows of `length` bytes and two result rows each on the device (LQADAPT_BATCH_READS overrides it)
u32 batch_reads()
{
	const char *v = getenv("LQADAPT_BATCH_READS");
	const long n = v ? atol(v) : 0;
	return n > 0 ? (u32)n : 262144u;
}

void run_adapter(AdaptDev &D, DBuf &win, u32 n_ends, u32 length, const DBuf &adp, u32 m, i32 *host_out)
{
	const u32 grid = n_ends < LQ_ADAPT_MAX_BLOCKS ? n_ends : LQ_ADAPT_MAX_BLOCKS;
	if (m > 64) LQ_LAUNCH(k_adapt<true>, grid, LQ_ADAPT_THREADS, D.stream, win.as<u8>(), n_ends, length, adp.as<u8>(), m, D.out.as<i32>());
	else LQ_LAUNCH(k_adapt<false>, grid, LQ_ADAPT_THREADS, D.stream, win.as<u8>(), n_ends, length, adp.as<u8>(), m, D.out.as<i32>());
	LQ_HIP_CHECK(hipGetLastError());
	LQ_HIP_CHECK(hipMemcpyAsync(host_out, D.out.p, (size_t)n_ends * 16, hipMemcpyDeviceToHost, D.stream));
}
} // namespace

extern "C" {

int lqadapt_reads(int device, uint32_t n, const uint8_t *seq, const uint64_t *seq_off,
                  const uint8_t *adp5, uint32_t len5, const uint8_t *adp3, uint32_t len3,
                  uint32_t length, int32_t *out5, int32_t *out3, char *errbuf, size_t errbuf_len)
{
	return lq_cabi::guarded(errbuf, errbuf_len, [&] {
		const bool do5 = adp5 && len5, do3 = adp3 && len3;
		if (!seq_off || (n && !seq) || (do5 && !out5) || (do3 && !out3)) throw std::invalid_argument("null buffers");
		if (length < 1 || length > LQ_ADAPT_MAXLEN) throw std::domain_error("adapter search window length outside [1, 4096]");
		if ((do5 && len5 > LQ_ADAPT_MAXADP) || (do3 && len3 > LQ_ADAPT_MAXADP)) throw std::domain_error("adapter longer than 32768 bases");
		for (u32 i = 0; i < n; ++i) if (seq_off[i + 1] < seq_off[i]) throw std::invalid_argument("seq_off is not ascending");
		for (u64 i = 0; i < (u64)n * 4; ++i) { if (do5) out5[i] = -1; if (do3) out3[i] = -1; }
		if (!do5 && !do3) return;
		std::vector<u32> idx;                                // the reads the reference aligns: at least 2 * length bases
		for (u32 i = 0; i < n; ++i) if (seq_off[i + 1] - seq_off[i] >= 2ULL * length) idx.push_back(i);
		if (idx.empty()) return;
		lq_cabi::select_device(device);
		AdaptDev D;
		LQ_HIP_CHECK(hipStreamCreate(&D.stream));
		if (do5) { D.adp5.ensure(len5); LQ_HIP_CHECK(hipMemcpyAsync(D.adp5.p, adp5, len5, hipMemcpyHostToDevice, D.stream)); }
		if (do3) { D.adp3.ensure(len3); LQ_HIP_CHECK(hipMemcpyAsync(D.adp3.p, adp3, len3, hipMemcpyHostToDevice, D.stream)); }
		const u32 B = batch_reads();
		std::vector<u8> h5, h3;
		std::vector<i32> r5, r3;
		for (size_t b0 = 0; b0 < idx.size(); b0 += B) {
			const u32 nb = (u32)std::min<size_t>(B, idx.size() - b0);
			const size_t wb = (size_t)nb * length;
			if (do5) { h5.resize(wb); r5.resize((size_t)nb * 4); D.win5.ensure(wb); }
			if (do3) { h3.resize(wb); r3.resize((size_t)nb * 4); D.win3.ensure(wb); }
			D.out.ensure((size_t)nb * 16);
			for (u32 k = 0; k < nb; ++k) {                   // 5': seq[:length], 3': seq[-length:]
				const u32 i = idx[b0 + k];
				if (do5) memcpy(&h5[(size_t)k * length], seq + seq_off[i], length);
				if (do3) memcpy(&h3[(size_t)k * length], seq + seq_off[i + 1] - length, length);
			}
			if (do5) {
				LQ_HIP_CHECK(hipMemcpyAsync(D.win5.p, h5.data(), wb, hipMemcpyHostToDevice, D.stream));
				run_adapter(D, D.win5, nb, length, D.adp5, len5, r5.data());
				LQ_HIP_CHECK(hipStreamSynchronize(D.stream));       // (D.out is reused by the 3' launch)
			}
			if (do3) {
				LQ_HIP_CHECK(hipMemcpyAsync(D.win3.p, h3.data(), wb, hipMemcpyHostToDevice, D.stream));
				run_adapter(D, D.win3, nb, length, D.adp3, len3, r3.data());
				LQ_HIP_CHECK(hipStreamSynchronize(D.stream));
			}
			for (u32 k = 0; k < nb; ++k) {
				const u32 i = idx[b0 + k];
				if (do5) memcpy(out5 + (size_t)i * 4, &r5[(size_t)k * 4], 16);
				if (do3) memcpy(out3 + (size_t)i * 4, &r3[(size_t)k * 4], 16);
			}
		}
	});
}

} // extern "C"
