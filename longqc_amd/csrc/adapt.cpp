// longqc_amd/csrc/adapt.cpp -- host side of the adapter search (lq_adapt.py:10-101) behind the C ABI of include/lqcov.h
// (lqadapt_reads).  The reads are a resident chunk (chunk.hpp); the host lists where the two end windows of every read of at least
// 2 * length bases lie in it, runs k_adapt (kernels_adapt.hpp) once per adapter and batch of reads, and scatters the per-end results
// back to read order.  Which
// reads the reference then skips or trims is decided by the caller (longqc_amd/adapter.py), where lq_adapt.py decides it.
#include "chunk.hpp"
#include "kernels_adapt.hpp"
#include <cstdlib>
#include <vector>

namespace {
// reads per batch: two window offsets and two result rows each on the device (LQADAPT_BATCH_READS overrides it)
u32 batch_reads()
{
	const char *v = getenv("LQADAPT_BATCH_READS");
	const long n = v ? atol(v) : 0;
	return n > 0 ? (u32)n : 262144u;
}

// one adapter against the n_ends windows whose offsets in the chunk are woff[]
void run_adapter(lqchunk &c, const std::vector<u64> &woff, u32 n_ends, u32 length, const DBuf &adp, u32 m, i32 *host_out)
{
	LQ_HIP_CHECK(hipMemcpyAsync(c.woff.p, woff.data(), (size_t)n_ends * 8, hipMemcpyHostToDevice, c.stream));
	const u32 grid = n_ends < LQ_ADAPT_MAX_BLOCKS ? n_ends : LQ_ADAPT_MAX_BLOCKS;
	if (m > 64) LQ_LAUNCH(k_adapt<true>, grid, LQ_ADAPT_THREADS, c.stream, c.seq.as<u8>(), c.woff.as<u64>(), n_ends, length, adp.as<u8>(), m, c.out.as<i32>());
	else LQ_LAUNCH(k_adapt<false>, grid, LQ_ADAPT_THREADS, c.stream, c.seq.as<u8>(), c.woff.as<u64>(), n_ends, length, adp.as<u8>(), m, c.out.as<i32>());
	LQ_HIP_CHECK(hipGetLastError());
	LQ_HIP_CHECK(hipMemcpyAsync(host_out, c.out.p, (size_t)n_ends * 16, hipMemcpyDeviceToHost, c.stream));
	LQ_HIP_CHECK(hipStreamSynchronize(c.stream));               // (c.woff and c.out are used again by the next launch)
}
} // namespace

// the search on a chunk's resident buffers (chunk.hpp): the windows are read where they lie, the first and the last `length`
// bases of every read of at least 2 * length
void lq_chunk_adapt(lqchunk &c, const u8 *adp5, u32 len5, const u8 *adp3, u32 len3, u32 length, i32 *out5, i32 *out3)
{
	const u32 n = c.n;
	const bool do5 = adp5 && len5, do3 = adp3 && len3;
	if ((do5 && !out5) || (do3 && !out3)) throw std::invalid_argument("null buffers");
	if (length < 1 || length > LQ_ADAPT_MAXLEN) throw std::domain_error("adapter search window length outside [1, 4096]");
	if ((do5 && len5 > LQ_ADAPT_MAXADP) || (do3 && len3 > LQ_ADAPT_MAXADP)) throw std::domain_error("adapter longer than 32768 bases");
	if (c.first_desc < n) throw std::invalid_argument("seq_off is not ascending");
	for (u64 i = 0; i < (u64)n * 4; ++i) { if (do5) out5[i] = -1; if (do3) out3[i] = -1; }
	if (!do5 && !do3) return;
	std::vector<u32> idx;                                    // the reads the reference aligns: at least 2 * length bases
	for (u32 i = 0; i < n; ++i) if (c.off[i + 1] - c.off[i] >= 2ULL * length) idx.push_back(i);
	if (idx.empty()) return;
	lq_chunk_ready(c);
	if (do5) { c.adp5.ensure(len5); LQ_HIP_CHECK(hipMemcpyAsync(c.adp5.p, adp5, len5, hipMemcpyHostToDevice, c.stream)); }
	if (do3) { c.adp3.ensure(len3); LQ_HIP_CHECK(hipMemcpyAsync(c.adp3.p, adp3, len3, hipMemcpyHostToDevice, c.stream)); }
	const u32 B = batch_reads();
	std::vector<u64> woff;
	std::vector<i32> r5, r3;
	for (size_t b0 = 0; b0 < idx.size(); b0 += B) {
		const u32 nb = (u32)std::min<size_t>(B, idx.size() - b0);
		woff.resize(nb);
		c.woff.ensure((size_t)nb * 8); c.out.ensure((size_t)nb * 16);
		if (do5) {                                           // 5': seq[:length]
			r5.resize((size_t)nb * 4);
			for (u32 k = 0; k < nb; ++k) woff[k] = c.off[idx[b0 + k]];
			run_adapter(c, woff, nb, length, c.adp5, len5, r5.data());
		}
		if (do3) {                                           // 3': seq[-length:]
			r3.resize((size_t)nb * 4);
			for (u32 k = 0; k < nb; ++k) woff[k] = c.off[idx[b0 + k] + 1] - length;
			run_adapter(c, woff, nb, length, c.adp3, len3, r3.data());
		}
		for (u32 k = 0; k < nb; ++k) {
			const u32 i = idx[b0 + k];
			if (do5) memcpy(out5 + (size_t)i * 4, &r5[(size_t)k * 4], 16);
			if (do3) memcpy(out3 + (size_t)i * 4, &r3[(size_t)k * 4], 16);
		}
	}
}

extern "C" {

int lqadapt_reads(int device, uint32_t n, const uint8_t *seq, const uint64_t *seq_off,
                  const uint8_t *adp5, uint32_t len5, const uint8_t *adp3, uint32_t len3,
                  uint32_t length, int32_t *out5, int32_t *out3, char *errbuf, size_t errbuf_len)
{
	return lq_cabi::guarded(errbuf, errbuf_len, [&] {
		if (!seq_off || (n && !seq)) throw std::invalid_argument("null buffers");
		lqchunk c;
		c.device = device;
		lq_chunk_set(c, n, seq, seq_off, nullptr);
		lq_chunk_adapt(c, adp5, len5, adp3, len3, length, out5, out3);
	});
}

} // extern "C"
