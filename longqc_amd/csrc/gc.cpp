// longqc_amd/csrc/gc.cpp -- host side of the GC fraction step (lq_gcfrac.py:25-48) behind the C ABI of include/lqcov.h
// (lqgc_reads).  The chunk's concatenated sequence is resident (chunk.hpp) and the kernels take it span by span (kernels_gc.hpp);
// the per-read counts, the drawn positions, the per-window counts and the per-read `kept` stay on the device for the whole call and
// come back once.
// The divisions and float32 roundings of the reference are the caller's (longqc_amd/gcfrac.py).
#include "chunk.hpp"
#include "kernels_gc.hpp"
#include <algorithm>
#include <cstdlib>
#include <vector>

static_assert(LQ_CHUNK_SEQ_TILE == LQ_GC_TILE, "the resident buffer holds whole tiles of k_gc_reads");

namespace {
// bytes of sequence per span, a multiple of LQ_GC_TILE (LQGC_BATCH_BASES overrides it).  128 MiB: a span that k_gc_reads has
// just streamed is still in the 256-MiB Infinity Cache when k_gc_windows reads a fifth of it again.
u64 batch_bases()
{
	const char *v = getenv("LQGC_BATCH_BASES");
	const long long n = v ? atoll(v) : 0;
	const u64 b = n > 0 ? (u64)n : (u64)128 << 20;
	return (b + LQ_GC_TILE - 1) / LQ_GC_TILE * LQ_GC_TILE;
}

u32 grid_for(u64 items, u64 per_block)
{
	const u64 g = (items + per_block - 1) / per_block;
	return (u32)(g < 1 ? 1 : g > LQ_GC_MAX_BLOCKS ? LQ_GC_MAX_BLOCKS : g);
}
} // namespace

// the counts on a chunk's resident buffers (chunk.hpp), span by span of the sequence
void lq_chunk_gc(lqchunk &c, u32 chunk_size, const u32 *k, const u64 *draw_off, const u32 *pos_in, u64 seed, u64 first_read,
                 u32 *gc, u32 *pos_out, u16 *win_gc, u32 *kept)
{
	const u32 n = c.n;
	const std::vector<u64> &off = c.off;                      // relative to the first base, as the kernels' spans are
	if ((n && !gc) || (k && (!draw_off || !kept))) throw std::invalid_argument("null buffers");
	if (chunk_size < 1 || chunk_size > LQ_GC_MAXCS) throw std::domain_error("chunk_size outside [1, 4096]");
	for (u32 i = 0; i < n; ++i) {
		if (i == c.first_desc) throw std::invalid_argument("seq_off is not ascending");
		if (off[i + 1] - off[i] >= (1ULL << 32)) throw std::domain_error("a read of 2^32 bases or more");
	}
	const u64 total = c.total;
	if (total && !c.resident && !c.h_seq) throw std::invalid_argument("null buffers");
	u64 n_draws = 0;
	if (k) {
		if (draw_off[0] != 0) throw std::invalid_argument("draw_off does not start at 0");
		for (u32 i = 0; i < n; ++i) {
			if (draw_off[i + 1] < draw_off[i] || draw_off[i + 1] - draw_off[i] != k[i]) throw std::invalid_argument("draw_off is not the prefix sum of k");
			if (k[i] > off[i + 1] - off[i]) throw std::invalid_argument("more draws than bases in a read");
		}
		n_draws = draw_off[n];
		if (n_draws && !win_gc) throw std::invalid_argument("null buffers");
		if (pos_in) for (u32 i = 0; i < n; ++i) {
			const u64 l = off[i + 1] - off[i];
			for (u64 d = draw_off[i]; d < draw_off[i + 1]; ++d) if (pos_in[d] >= l) throw std::invalid_argument("a position outside its read");
		}
	}
	if (n == 0) return;
	for (u32 i = 0; i < n; ++i) gc[i] = 0;
	if (k) memcpy(kept, k, (size_t)n * 4);
	if (total == 0) return;                                   // (no bases: no draws either, k[i] <= l)

	lq_chunk_ready(c);
	c.gc.ensure((size_t)n * 4);
	LQ_HIP_CHECK(hipMemsetAsync(c.gc.p, 0, (size_t)n * 4, c.stream));
	if (n_draws) {
		c.draw_off.ensure((size_t)(n + 1) * 8);
		LQ_HIP_CHECK(hipMemcpyAsync(c.draw_off.p, draw_off, (size_t)(n + 1) * 8, hipMemcpyHostToDevice, c.stream));
		c.kept.ensure((size_t)n * 4);
		LQ_HIP_CHECK(hipMemcpyAsync(c.kept.p, k, (size_t)n * 4, hipMemcpyHostToDevice, c.stream));
		c.win.ensure((size_t)n_draws * 2);
		LQ_HIP_CHECK(hipMemsetAsync(c.win.p, 0, (size_t)n_draws * 2, c.stream));
		c.pos.ensure((size_t)n_draws * 4);
		if (pos_in) LQ_HIP_CHECK(hipMemcpyAsync(c.pos.p, pos_in, (size_t)n_draws * 4, hipMemcpyHostToDevice, c.stream));
		else {
			LQ_LAUNCH(k_gc_draw, grid_for(n_draws, LQ_GC_THREADS), LQ_GC_THREADS, c.stream, c.d_off.as<u64>(), c.draw_off.as<u64>(), n, (u64)seed, (u64)first_read, c.pos.as<u32>());
			LQ_HIP_CHECK(hipGetLastError());
		}
	}
	// the resident buffer holds whole tiles (lq_chunk_ready): span [b0, b1) is c.seq + b0, and a window that starts inside it is read to its end
	const u64 B = batch_bases();
	for (u64 b0 = 0; b0 < total; b0 += B) {
		const u64 b1 = std::min(total, b0 + B);
		LQ_LAUNCH(k_gc_reads, grid_for((b1 - b0 + LQ_GC_TILE - 1) / LQ_GC_TILE, LQ_GC_THREADS / 64), LQ_GC_THREADS, c.stream,
		          c.seq.as<u8>() + b0, b0, b1, c.d_off.as<u64>(), n, c.gc.as<u32>());
		LQ_HIP_CHECK(hipGetLastError());
		if (n_draws) {
			// the reads that hold bytes b0 and b1 - 1 (empty reads hold none), and their draws
			const u32 r_lo = (u32)(std::upper_bound(off.begin(), off.end(), b0) - off.begin()) - 1;
			const u32 r_hi = (u32)(std::upper_bound(off.begin(), off.end(), b1 - 1) - off.begin()) - 1;
			const u64 d_lo = draw_off[r_lo], d_hi = draw_off[r_hi + 1];
			if (d_hi > d_lo) {
				LQ_LAUNCH(k_gc_windows, grid_for(d_hi - d_lo, LQ_GC_THREADS / 16), LQ_GC_THREADS, c.stream, c.seq.as<u8>() + b0, b0, b1, c.d_off.as<u64>(),
				          c.draw_off.as<u64>(), n, c.pos.as<u32>(), (u32)chunk_size, d_lo, d_hi, c.win.as<u16>(), c.kept.as<u32>());
				LQ_HIP_CHECK(hipGetLastError());
			}
		}
	}
	LQ_HIP_CHECK(hipMemcpyAsync(gc, c.gc.p, (size_t)n * 4, hipMemcpyDeviceToHost, c.stream));
	if (n_draws) {
		LQ_HIP_CHECK(hipMemcpyAsync(kept, c.kept.p, (size_t)n * 4, hipMemcpyDeviceToHost, c.stream));
		LQ_HIP_CHECK(hipMemcpyAsync(win_gc, c.win.p, (size_t)n_draws * 2, hipMemcpyDeviceToHost, c.stream));
		if (pos_out) LQ_HIP_CHECK(hipMemcpyAsync(pos_out, c.pos.p, (size_t)n_draws * 4, hipMemcpyDeviceToHost, c.stream));
	}
	LQ_HIP_CHECK(hipStreamSynchronize(c.stream));
	for (u32 i = 0; i < n && n_draws; ++i)                    // counts at or after the position the walk stops at are not reported
		for (u64 d = draw_off[i] + kept[i]; d < draw_off[i + 1]; ++d) win_gc[d] = 0;
}

extern "C" {

int lqgc_reads(int device, uint32_t n, const uint8_t *seq, const uint64_t *seq_off, uint32_t chunk_size, const uint32_t *k,
               const uint64_t *draw_off, const uint32_t *pos_in, uint64_t seed, uint64_t first_read, uint32_t *gc,
               uint32_t *pos_out, uint16_t *win_gc, uint32_t *kept, char *errbuf, size_t errbuf_len)
{
	return lq_cabi::guarded(errbuf, errbuf_len, [&] {
		if (!seq_off) throw std::invalid_argument("null buffers");
		lqchunk c;
		c.device = device;
		lq_chunk_set(c, n, seq, seq_off, nullptr);
		lq_chunk_gc(c, chunk_size, k, draw_off, pos_in, seed, first_read, gc, pos_out, win_gc, kept);
	});
}

} // extern "C"
