// longqc_amd/csrc/dust.cpp -- host side of the low-complexity table: the reference's `sdust` binary
// (sdust.c:181-222) behind the C ABI of include/lqcov.h (lqsdust_*).  Reads go to the device as ASCII (a resident chunk, chunk.hpp), one
// thread walks one read (kernels_dust.hpp); rows are formatted on the host with libc/libm like the reference, or -- opt-in, lqsdust_format and
// lqchunk_sdust_table -- on the device (kernels_dust_table.hpp), where the host takes only the mean qualities the device does not vouch for.
#include "engine.hpp"
#include "kernels_dust.hpp"
#include "kernels_dust_split.hpp"
#include "kernels_dust_table.hpp"
#include "fastx.hpp"
#include "chunk.hpp"
using lq_cabi::guarded;
using lq_cabi::select_device;
#include <cstdio>
#include <cstring>
#include <cmath>
#include <cstdlib>
#include <chrono>
#include <thread>
#include <mutex>
#include <condition_variable>
#include <exception>
#include <algorithm>

static inline dim3 nblk_d(u64 n, u32 b) { return dim3((unsigned)((n + b - 1) / b)); }

// the scan on a chunk's resident buffers (chunk.hpp): one thread walks one read
void lq_chunk_sdust(lqchunk &c, int W, int T, u32 *masked, double *psum, u32 *qv)
{
	if (W < 3 || W > 66) throw std::domain_error("sdust window outside [3, 66] (the window ring holds 64 words; the reference's default is 64)");
	const u32 n = c.n;
	c.dust_done = false; c.cols_done = false;
	if (n == 0) { c.dust_done = true; return; }
	for (u32 i = 0; i < n; ++i) if (c.off[i + 1] - c.off[i] > 0x7fffffffULL) throw std::domain_error("read longer than 2^31-1 bases");
	lq_chunk_ready(c);
	const u32 n_thr = (u32)std::min<u64>(((u64)n + LQ_DUST_THREADS - 1) / LQ_DUST_THREADS * LQ_DUST_THREADS, LQ_DUST_MAX_THREADS);
	c.pi.ensure((u64)n_thr * LQ_DUST_PCAP * sizeof(DustPI));
	c.masked.ensure(n * 4 + 4); c.psum.ensure(n * 8 + 8); c.qv.ensure(n * 4 + 4);
	if (!c.tab_ready) {
		double tab[127]; lq_make_q2p(tab);
		c.q2p.ensure(127 * 8);
		LQ_HIP_CHECK(hipMemcpyAsync(c.q2p.p, tab, sizeof(tab), hipMemcpyHostToDevice, c.stream));
		LQ_HIP_CHECK(hipStreamSynchronize(c.stream));
		c.tab_ready = true;
	}
	LQ_LAUNCH(k_sdust, nblk_d(n_thr, LQ_DUST_THREADS), LQ_DUST_THREADS, c.stream, c.seq.as<u8>(), c.has_qual ? c.qual.as<u8>() : (const u8*)nullptr,
	          c.d_off.as<u64>(), n, (i32)W, (i32)T, c.q2p.as<double>(), c.pi.as<DustPI>(), c.masked.as<u32>(), c.psum.as<double>(), c.qv.as<u32>());
	LQ_HIP_CHECK(hipGetLastError());
	if (masked) {                                              // (null: the results stay on the device, for lq_chunk_sdust_table)
		LQ_HIP_CHECK(hipMemcpyAsync(masked, c.masked.p, n * 4, hipMemcpyDeviceToHost, c.stream));
		LQ_HIP_CHECK(hipMemcpyAsync(psum, c.psum.p, n * 8, hipMemcpyDeviceToHost, c.stream));
		LQ_HIP_CHECK(hipMemcpyAsync(qv, c.qv.p, n * 4, hipMemcpyDeviceToHost, c.stream));
	}
	LQ_HIP_CHECK(hipStreamSynchronize(c.stream));
	c.dust_done = true;
}

// ---- the scan in pieces (kernels_dust_split.hpp) -----------------------------------------------------------------------------
static void dust_checks(const lqchunk &c, int W)
{
	if (W < 3 || W > 66) throw std::domain_error("sdust window outside [3, 66] (the window ring holds 64 words; the reference's default is 64)");
	for (u32 i = 0; i < c.n; ++i) if (c.off[i + 1] - c.off[i] > 0x7fffffffULL) throw std::domain_error("read longer than 2^31-1 bases");
}

static u32 dust_piece(const lqchunk &c, int W, u32 piece)
{
	if (c.total > 0xffffffffULL) throw std::domain_error("sdust in pieces: a chunk of 2^32 bases or more (the mask's bit numbers have 32 bits)");
	if (piece == 0) piece = LQ_DUST_SPLIT_PIECE;
	if (piece < (u32)(2 * W + 2)) throw std::invalid_argument("sdust piece shorter than 2 W + 2 bases");
	return std::min<u32>(piece, 0x40000000u);                   // (a longer piece cuts no read)
}

static void dust_q2p(lqchunk &c)
{
	if (c.tab_ready) return;
	double tab[127]; lq_make_q2p(tab);
	c.q2p.ensure(127 * 8);
	LQ_HIP_CHECK(hipMemcpyAsync(c.q2p.p, tab, sizeof(tab), hipMemcpyHostToDevice, c.stream));
	LQ_HIP_CHECK(hipStreamSynchronize(c.stream));
	c.tab_ready = true;
}

// classify, cut and walk the pieces: afterwards c.dmask holds the mask of the unflagged reads, c.dflag / c.h_dflag the flags and c.ditem
// the items before every read.  Everything is queued on c.stream; the flags have come back.  -> the number of flagged reads.  all_lengths:
// a short read is not flagged (the intervals: the pieces are the only walk that gives them, and a read of one piece is served as well)
static u32 dust_mask(lqchunk &c, int W, int T, u32 piece, bool all_lengths, std::vector<u32> *serial)
{
	const u32 n = c.n;
	c.iv_valid = false;                                         // (the flags and the mask that the kept intervals came from go)
	c.dflag.ensure(n + 4); c.h_dflag.resize(n);
	LQ_HIP_CHECK(hipMemsetAsync(c.dflag.p, 0, n, c.stream));
	const u64 n_tiles = (c.total + LQ_DUST_SPLIT_TILE - 1) / LQ_DUST_SPLIT_TILE;
	const u32 cgrid = (u32)std::min<u64>(std::max<u64>(std::max<u64>((n_tiles + 3) / 4, ((u64)n + LQ_DUST_SPLIT_THREADS - 1) / LQ_DUST_SPLIT_THREADS), 1), LQ_DUST_SPLIT_MAX_BLOCKS);
	LQ_LAUNCH(k_sdust_classify, cgrid, LQ_DUST_SPLIT_THREADS, c.stream, c.seq.as<u8>(), c.d_off.as<u64>(), n, all_lengths ? (u64)0 : LQ_DUST_SPLIT_MIN(piece), c.dflag.as<u8>());
	LQ_HIP_CHECK(hipGetLastError());
	LQ_HIP_CHECK(hipMemcpyAsync(c.h_dflag.data(), c.dflag.p, n, hipMemcpyDeviceToHost, c.stream));
	LQ_HIP_CHECK(hipStreamSynchronize(c.stream));
	u32 k = 0;
	for (u32 i = 0; i < n; ++i) if (c.h_dflag[i]) { ++k; if (serial) serial->push_back(i); }
	std::vector<u64> item((size_t)n + 1);
	item[0] = 0;
	for (u32 i = 0; i < n; ++i) item[i + 1] = item[i] + (c.h_dflag[i] ? 0 : (c.off[i + 1] - c.off[i] + piece - 1) / piece);
	if (item[n] > 0x7fffffffULL) throw std::domain_error("more than 2^31-1 pieces in one chunk");
	const u64 n_items = item[n], n_words = (c.total + 31) / 32 + 1;
	c.dmask.ensure(n_words * 4);
	LQ_HIP_CHECK(hipMemsetAsync(c.dmask.p, 0, n_words * 4, c.stream));
	if (n_items) {
		c.ditem.ensure(((size_t)n + 1) * 8);
		LQ_HIP_CHECK(hipMemcpyAsync(c.ditem.p, item.data(), ((size_t)n + 1) * 8, hipMemcpyHostToDevice, c.stream));
		const u32 n_thr = (u32)std::min<u64>((n_items + LQ_DUST_THREADS - 1) / LQ_DUST_THREADS * LQ_DUST_THREADS, LQ_DUST_SPLIT_MAX_THREADS);
		c.pi.ensure((u64)n_thr * LQ_DUST_PCAP * sizeof(DustPI));
		LQ_LAUNCH(k_sdust_pieces, nblk_d(n_thr, LQ_DUST_THREADS), LQ_DUST_THREADS, c.stream, c.seq.as<u8>(), c.d_off.as<u64>(), c.ditem.as<u64>(), n, (u32)n_items,
		          piece, (i32)W, (i32)T, c.pi.as<DustPI>(), c.dmask.as<u32>());
		LQ_HIP_CHECK(hipGetLastError());
		LQ_HIP_CHECK(hipStreamSynchronize(c.stream));             // (`item` dies here)
	}
	return k;
}

void lq_chunk_sdust_split(lqchunk &c, int W, int T, u32 piece, u32 *masked, double *psum, u32 *qv, u32 *n_serial)
{
	dust_checks(c, W);
	piece = dust_piece(c, W, piece);
	const u32 n = c.n;
	if (n_serial) *n_serial = 0;
	c.dust_done = false; c.cols_done = false;
	if (n == 0) { c.dust_done = true; return; }
	lq_chunk_ready(c);
	if (!c.stream2) LQ_HIP_CHECK(hipStreamCreate(&c.stream2));
	dust_q2p(c);
	c.masked.ensure(n * 4 + 4); c.psum.ensure(n * 8 + 8); c.qv.ensure(n * 4 + 4);
	// the quality columns need nothing of the rest: a launch of their own on the second stream, beside the pieces
	const u32 q_thr = (u32)std::min<u64>(((u64)n + LQ_DUST_THREADS - 1) / LQ_DUST_THREADS * LQ_DUST_THREADS, LQ_DUST_MAX_THREADS);
	LQ_LAUNCH(k_sdust_qual, nblk_d(q_thr, LQ_DUST_THREADS), LQ_DUST_THREADS, c.stream2, c.has_qual ? c.qual.as<u8>() : (const u8*)nullptr, c.d_off.as<u64>(), n,
	          c.q2p.as<double>(), c.psum.as<double>(), c.qv.as<u32>());
	LQ_HIP_CHECK(hipGetLastError());
	std::vector<u32> serial;
	std::vector<u64> soff;
	try {
		const u32 k = dust_mask(c, W, T, piece, false, &serial);
		if (n_serial) *n_serial = k;
		if (k) {                                                  // the flagged reads, set one behind the other, through k_sdust as it is
			soff.resize((size_t)k + 1);
			soff[0] = 0;
			for (u32 j = 0; j < k; ++j) soff[j + 1] = soff[j] + (c.off[serial[j] + 1] - c.off[serial[j]]);
			c.slist.ensure((size_t)k * 4); c.soff.ensure(((size_t)k + 1) * 8); c.sseq.ensure(soff[k] + 16);
			c.smasked.ensure(k * 4 + 4); c.spsum.ensure(k * 8 + 8); c.sqv.ensure(k * 4 + 4);
			LQ_HIP_CHECK(hipMemcpyAsync(c.slist.p, serial.data(), (size_t)k * 4, hipMemcpyHostToDevice, c.stream));
			LQ_HIP_CHECK(hipMemcpyAsync(c.soff.p, soff.data(), ((size_t)k + 1) * 8, hipMemcpyHostToDevice, c.stream));
			LQ_LAUNCH(k_sdust_compact, std::min<u32>(k, LQ_DUST_SPLIT_MAX_BLOCKS), LQ_DUST_SPLIT_THREADS, c.stream, c.seq.as<u8>(), c.d_off.as<u64>(),
			          c.slist.as<u32>(), c.soff.as<u64>(), k, c.sseq.as<u8>());
			const u32 n_thr = (u32)std::min<u64>(((u64)k + LQ_DUST_THREADS - 1) / LQ_DUST_THREADS * LQ_DUST_THREADS, LQ_DUST_MAX_THREADS);
			c.pi.ensure((u64)n_thr * LQ_DUST_PCAP * sizeof(DustPI));
			LQ_LAUNCH(k_sdust, nblk_d(n_thr, LQ_DUST_THREADS), LQ_DUST_THREADS, c.stream, c.sseq.as<u8>(), (const u8*)nullptr, c.soff.as<u64>(), k, (i32)W, (i32)T,
			          c.q2p.as<double>(), c.pi.as<DustPI>(), c.smasked.as<u32>(), c.spsum.as<double>(), c.sqv.as<u32>());
			LQ_LAUNCH(k_sdust_scatter, std::min<u32>((k + LQ_DUST_SPLIT_THREADS - 1) / LQ_DUST_SPLIT_THREADS, LQ_DUST_SPLIT_MAX_BLOCKS), LQ_DUST_SPLIT_THREADS, c.stream,
			          c.smasked.as<u32>(), c.slist.as<u32>(), k, c.masked.as<u32>());
			LQ_HIP_CHECK(hipGetLastError());
		}
		if (k < n) {
			LQ_LAUNCH(k_sdust_mask_count, (u32)std::min<u64>(((u64)n + 3) / 4, LQ_DUST_SPLIT_MAX_BLOCKS), LQ_DUST_SPLIT_THREADS, c.stream, c.dmask.as<u32>(), c.d_off.as<u64>(),
			          c.dflag.as<u8>(), n, c.masked.as<u32>());
			LQ_HIP_CHECK(hipGetLastError());
		}
		if (masked) {
			LQ_HIP_CHECK(hipMemcpyAsync(masked, c.masked.p, n * 4, hipMemcpyDeviceToHost, c.stream));
			LQ_HIP_CHECK(hipMemcpyAsync(psum, c.psum.p, n * 8, hipMemcpyDeviceToHost, c.stream2));
			LQ_HIP_CHECK(hipMemcpyAsync(qv, c.qv.p, n * 4, hipMemcpyDeviceToHost, c.stream2));
		}
	} catch (...) {                                              // (nothing of this call stays queued behind the caller's buffers)
		(void)hipStreamSynchronize(c.stream); (void)hipStreamSynchronize(c.stream2);
		throw;
	}
	LQ_HIP_CHECK(hipStreamSynchronize(c.stream));                 // (`serial` and `soff` die here)
	LQ_HIP_CHECK(hipStreamSynchronize(c.stream2));
	c.dust_done = true;
}

void lq_chunk_sdust_intervals(lqchunk &c, int W, int T, u32 piece)
{
	dust_checks(c, W);
	piece = dust_piece(c, W, piece);
	const u32 n = c.n;
	if (n == 0) { c.h_iv.clear(); c.h_ivoff.assign(1, 0); c.h_dflag.clear(); c.iv_valid = false; return; }
	// the second of the two calls (iv == NULL, then iv != NULL) finds the first one's runs: the same W, T and piece on the same reads
	if (c.iv_valid && c.iv_W == W && c.iv_T == T && c.iv_piece == piece) return;
	lq_chunk_ready(c);
	dust_mask(c, W, T, piece, true, nullptr);
	const u64 n_words = (c.total + 31) / 32 + 1;
	std::vector<u32> m((size_t)n_words);
	LQ_HIP_CHECK(hipMemcpyAsync(m.data(), c.dmask.p, n_words * 4, hipMemcpyDeviceToHost, c.stream));
	LQ_HIP_CHECK(hipStreamSynchronize(c.stream));
	c.h_iv.clear(); c.h_ivoff.assign((size_t)n + 1, 0);
	for (u32 r = 0; r < n; ++r) {
		const u64 a = c.off[r], b = c.off[r + 1];
		if (!c.h_dflag[r])
			for (u64 g = a; g < b;) {                             // word-wise: the next set bit, then the next clear one
				u32 w = m[g >> 5] >> (g & 31);
				if (!w) { g = (g | 31) + 1; continue; }
				g += __builtin_ctz(w);
				if (g >= b) break;
				u64 e = g;
				while (e < b) {
					const u32 v = ~(m[e >> 5] >> (e & 31));           // (the shift brings zeros in: they end the run at the word's end at the latest)
					const u32 room = 32 - (u32)(e & 31), z = v ? (u32)__builtin_ctz(v) : 32u;
					if (z < room) { e += z; break; }
					e += room;
				}
				if (e > b) e = b;
				c.h_iv.push_back((g - a) << 32 | (e - a));
				g = e;
			}
		c.h_ivoff[r + 1] = c.h_iv.size();
	}
	c.iv_valid = true; c.iv_W = W; c.iv_T = T; c.iv_piece = piece;
}

// ---- the table as text (kernels_dust_table.hpp) ------------------------------------------------------------------------------
// meanQ(qual.s, qual.l) of the reference (lqutils.c:51-58) with libm, 0.0 / 0 without qualities: lqsdust_main's rows and the rows the
// device does not vouch for
static double dust_meanq(bool has_q, double psum, int len)
{
	volatile double num = has_q ? psum : 0.0; volatile int ql = has_q ? len : 0;
	return -10 * log10(num / ql);
}

// the rows of one mini-batch as the reference prints them (sdust.c:211-217)
static void dust_print_rows(FILE *o, const ReadBatch &rb, const u32 *masked, const double *psum, const u32 *qv)
{
	const u32 n = rb.size();
	for (u32 i = 0; i < n; ++i) {
		const int len = (int)(rb.seq_off[i + 1] - rb.seq_off[i]);
		const bool has_q = rb.any_qual && len > 0 && rb.qual[rb.seq_off[i]] != 0;
		const double mq = dust_meanq(has_q, psum[i], len);
		volatile double m = (double)masked[i]; volatile int sl = len;
		fprintf(o, "%s\t%d\t%d\t%.3f\t%.3f\t%d\n", rb.name(i), (int)masked[i], len, m / sl, mq, (int)qv[i]);
	}
}

namespace {
static_assert(sizeof(lqsdust_stats) == LQSDUST_STATS_WORDS * 8, "lqsdust_stats is LQSDUST_STATS_WORDS words");
struct DustTabIn {                                            // device arrays of n rows: len or off, has_q or qual (kernels_dust_table.hpp)
	u32 n; const u32 *masked, *len; const u64 *off; const double *psum; const u8 *has_q, *qual; const u32 *q7;
};

// arrays on the device -> the text on the host.  Nothing is written to out or excl unless both have room
void dust_table_queued(LqDustTab &tb, hipStream_t stream, const DustTabIn &in, const char *names, const u64 *name_off, double window, u8 *out, u64 out_cap,
                u64 *out_len, u64 *stats, u32 *excl, u64 excl_cap)
{
	const u32 n = in.n;
	*out_len = 0;
	for (u32 w = 0; w < LQSDUST_STATS_WORDS; ++w) stats[w] = 0;
	if (!n) return;
	if (names && !name_off) throw std::invalid_argument("null buffers");
	if (!(window >= 0)) throw std::invalid_argument("window must not be negative");
	if (window == 0) window = LQ_DTAB_WINDOW;
	// the names: the bytes names[blob0 .. blob1), where each starts in them, and its length
	std::vector<u64> noff(n, 0);
	std::vector<u32> nlen(n, 0);
	u64 blob0 = LQ_U64MAX, blob1 = 0;
	for (u32 i = 0; names && i < n; ++i) blob0 = std::min(blob0, name_off[i]);
	for (u32 i = 0; names && i < n; ++i) {
		const size_t l = strlen(names + name_off[i]);
		if (l > 0xffffffULL) throw std::domain_error("a name of 2^24 bytes or more");
		noff[i] = name_off[i] - blob0; nlen[i] = (u32)l;
		blob1 = std::max(blob1, name_off[i] + l);
	}
	const u64 blob = names ? blob1 - blob0 : 0;
	tb.names.ensure((size_t)blob + 16); tb.noff.ensure((size_t)n * 8); tb.nlen.ensure((size_t)n * 4);
	tb.fthou.ensure((size_t)n * 8); tb.qthou.ensure((size_t)n * 8); tb.meta.ensure((size_t)n * 4); tb.rbytes.ensure(((size_t)n + 1) * 4);
	tb.rec.ensure(((size_t)n + 1) * 8); tb.unv.ensure((size_t)n * sizeof(DustUnv)); tb.ex1.ensure((size_t)n * 4); tb.ex2.ensure((size_t)n * 4);
	tb.st.ensure(LQ_DTAB_ST_WORDS * 8);
	if (blob) LQ_HIP_CHECK(hipMemcpyAsync(tb.names.p, names + blob0, (size_t)blob, hipMemcpyHostToDevice, stream));
	LQ_HIP_CHECK(hipMemcpyAsync(tb.noff.p, noff.data(), (size_t)n * 8, hipMemcpyHostToDevice, stream));
	LQ_HIP_CHECK(hipMemcpyAsync(tb.nlen.p, nlen.data(), (size_t)n * 4, hipMemcpyHostToDevice, stream));
	LQ_HIP_CHECK(hipMemsetAsync(tb.st.p, 0, LQ_DTAB_ST_WORDS * 8, stream));
	LQ_HIP_CHECK(hipMemsetAsync(tb.rbytes.as<u32>() + n, 0, 4, stream));
	const u32 grid = (u32)std::min<u64>(((u64)n + LQ_DTAB_THREADS - 1) / LQ_DTAB_THREADS, LQ_DTAB_MAX_BLOCKS);
	LQ_LAUNCH(k_sdust_rows, grid, LQ_DTAB_THREADS, stream, n, tb.nlen.as<u32>(), in.masked, in.len, in.off, in.psum, in.has_q, in.qual, in.q7, window,
	          tb.fthou.as<u64>(), tb.qthou.as<u64>(), tb.meta.as<u32>(), tb.rbytes.as<u32>(), tb.unv.as<DustUnv>(), tb.ex1.as<u32>(), tb.ex2.as<u32>(),
	          tb.st.as<unsigned long long>());
	LQ_HIP_CHECK(hipGetLastError());
	u64 st[LQ_DTAB_ST_WORDS];
	LQ_HIP_CHECK(hipMemcpyAsync(st, tb.st.p, sizeof(st), hipMemcpyDeviceToHost, stream));
	LQ_HIP_CHECK(hipStreamSynchronize(stream));                 // (noff and nlen die here)
	const u64 k = st[LQ_DTAB_ST_UNV], e1 = st[LQ_DTAB_ST_EX1], e2 = st[LQ_DTAB_ST_EX2];
	if (k > n || e1 > n || e2 > n) throw std::logic_error("the table's lists are longer than the chunk");
	std::vector<DustPatch> patch;
	if (k) {                                                      // the rows the device does not vouch for: meanQ with libm, the same rounding
		std::vector<DustUnv> unv((size_t)k);
		LQ_HIP_CHECK(hipMemcpyAsync(unv.data(), tb.unv.p, (size_t)k * sizeof(DustUnv), hipMemcpyDeviceToHost, stream));
		LQ_HIP_CHECK(hipStreamSynchronize(stream));
		patch.resize((size_t)k);
		for (u64 j = 0; j < k; ++j) {
			patch[j].idx = unv[j].idx;
			patch[j].qcls = lq_fmt3_round(dust_meanq(true, unv[j].psum, (int)unv[j].len), &patch[j].qthou);
			if (LQ_F3_CLASS(patch[j].qcls) == LQ_F3_BIG) throw std::domain_error("a mean quality of 2^50 or more");
		}
		tb.patch.ensure((size_t)k * sizeof(DustPatch));
		LQ_HIP_CHECK(hipMemcpyAsync(tb.patch.p, patch.data(), (size_t)k * sizeof(DustPatch), hipMemcpyHostToDevice, stream));
		const u32 pgrid = (u32)std::min<u64>((k + LQ_DTAB_THREADS - 1) / LQ_DTAB_THREADS, LQ_DTAB_MAX_BLOCKS);
		LQ_LAUNCH(k_sdust_patch, pgrid, LQ_DTAB_THREADS, stream, (u32)k, tb.patch.as<DustPatch>(), tb.qthou.as<u64>(), tb.meta.as<u32>(), tb.rbytes.as<u32>());
		LQ_HIP_CHECK(hipGetLastError());
	}
	tb.prim.stream = stream;
	tb.prim.exclusive_scan_u32_u64(tb.rbytes.as<u32>(), tb.rec.as<u64>(), (size_t)n + 1);
	u64 total = 0;
	LQ_HIP_CHECK(hipMemcpyAsync(&total, tb.rec.as<u64>() + n, 8, hipMemcpyDeviceToHost, stream));
	LQ_HIP_CHECK(hipStreamSynchronize(stream));                 // (`patch` dies here)
	*out_len = total;
	stats[0] = n; stats[1] = total; stats[2] = st[LQ_DTAB_ST_MASKED]; stats[3] = st[LQ_DTAB_ST_Q7]; stats[4] = k; stats[5] = e1 + e2; stats[6] = e1;
	if (total > out_cap) throw std::invalid_argument("out_cap is smaller than the table");
	if (excl && e1 + e2 > excl_cap) throw std::invalid_argument("excl_cap is smaller than the exclusion lists");
	if (!out) throw std::invalid_argument("null buffers");
	tb.text.ensure((size_t)total + 16);
	LQ_LAUNCH(k_sdust_text, grid, LQ_DTAB_THREADS, stream, n, tb.names.as<u8>(), tb.noff.as<u64>(), tb.nlen.as<u32>(), in.masked, in.len, in.off, in.q7,
	          tb.fthou.as<u64>(), tb.qthou.as<u64>(), tb.meta.as<u32>(), tb.rec.as<u64>(), tb.text.as<u8>());
	LQ_HIP_CHECK(hipGetLastError());
	LQ_HIP_CHECK(hipMemcpyAsync(out, tb.text.p, (size_t)total, hipMemcpyDeviceToHost, stream));
	if (excl && e1) LQ_HIP_CHECK(hipMemcpyAsync(excl, tb.ex1.p, (size_t)e1 * 4, hipMemcpyDeviceToHost, stream));
	if (excl && e2) LQ_HIP_CHECK(hipMemcpyAsync(excl + e1, tb.ex2.p, (size_t)e2 * 4, hipMemcpyDeviceToHost, stream));
	LQ_HIP_CHECK(hipStreamSynchronize(stream));
	if (excl) { std::sort(excl, excl + e1); std::sort(excl + e1, excl + e1 + e2); }    // (the atomics' order -> file order)
}

// (its copies come from and go to memory of this call and of the caller: nothing of a call that throws stays queued behind them)
void dust_table(LqDustTab &tb, hipStream_t stream, const DustTabIn &in, const char *names, const u64 *name_off, double window, u8 *out, u64 out_cap,
                u64 *out_len, u64 *stats, u32 *excl, u64 excl_cap)
{
	try { dust_table_queued(tb, stream, in, names, name_off, window, out, out_cap, out_len, stats, excl, excl_cap); }
	catch (...) { (void)hipStreamSynchronize(stream); throw; }
}
} // namespace

void lq_chunk_sdust_table(lqchunk &c, const char *names, const u64 *name_off, u8 *out, u64 out_cap, u64 *out_len, u64 *stats, u32 *excl, u64 excl_cap)
{
	if (!c.dust_done) throw std::logic_error("no scan of the chunk loaded now (lqchunk_sdust, lqchunk_sdust_split)");
	lq_cabi::select_device(c.device);
	const DustTabIn in = {c.n, c.masked.as<u32>(), nullptr, c.d_off.as<u64>(), c.psum.as<double>(), nullptr, c.has_qual ? c.qual.as<u8>() : (const u8*)nullptr, c.qv.as<u32>()};
	c.cols_done = false;
	dust_table(c.tb, c.stream, in, names, name_off, 0, out, out_cap, out_len, stats, excl, excl_cap);
	c.cols_done = true;
}

void lq_chunk_sdust_columns(lqchunk &c, u32 *frac_thou, i32 *qv_thou)
{
	if (!c.dust_done || !c.cols_done) throw std::logic_error("no table of the chunk loaded now (lqchunk_sdust_table)");
	const u32 n = c.n;
	if (!n) return;
	if (!frac_thou || !qv_thou) throw std::invalid_argument("null buffers");
	lq_cabi::select_device(c.device);
	LqDustTab &tb = c.tb;
	tb.cfrac.ensure((size_t)n * 4); tb.cqv.ensure((size_t)n * 4);
	try {
		LQ_HIP_CHECK(hipMemsetAsync(tb.st.p, 0, 4, c.stream));
		const u32 grid = (u32)std::min<u64>(((u64)n + LQ_DTAB_THREADS - 1) / LQ_DTAB_THREADS, LQ_DTAB_MAX_BLOCKS);
		LQ_LAUNCH(k_sdust_columns, grid, LQ_DTAB_THREADS, c.stream, n, tb.fthou.as<u64>(), tb.qthou.as<u64>(), tb.meta.as<u32>(), tb.cfrac.as<u32>(), tb.cqv.as<i32>(),
		          tb.st.as<u32>());
		LQ_HIP_CHECK(hipGetLastError());
		u32 bad = 0;
		LQ_HIP_CHECK(hipMemcpyAsync(&bad, tb.st.p, 4, hipMemcpyDeviceToHost, c.stream));
		LQ_HIP_CHECK(hipMemcpyAsync(frac_thou, tb.cfrac.p, (size_t)n * 4, hipMemcpyDeviceToHost, c.stream));
		LQ_HIP_CHECK(hipMemcpyAsync(qv_thou, tb.cqv.p, (size_t)n * 4, hipMemcpyDeviceToHost, c.stream));
		LQ_HIP_CHECK(hipStreamSynchronize(c.stream));
		if (bad) throw std::domain_error("a column value that is infinite or does not fit 31 bits of thousandths");
	} catch (...) { (void)hipStreamSynchronize(c.stream); throw; }
}

extern "C" {

uint32_t lqsdust_fmt3(double x, uint64_t *thousandths)
{
	u64 t = 0;
	const u32 c = lq_fmt3_round(x, &t);
	if (thousandths) *thousandths = t;
	return c;
}

int lqsdust_format_lists(int device, uint32_t n, const char *names, const uint64_t *name_off, const uint32_t *masked, const uint32_t *len,
                         const double *qual_psum, const uint8_t *has_q, const uint32_t *n_above_q7, double window, uint8_t *out, uint64_t out_cap,
                         uint64_t *out_len, lqsdust_stats *stats, uint32_t *excl, uint64_t excl_cap, char *errbuf, size_t errbuf_len)
{
	return guarded(errbuf, errbuf_len, [&] {
		if (!out_len || (n && (!masked || !len || !qual_psum || !n_above_q7))) throw std::invalid_argument("null buffers");
		lq_cabi::ScopedStream stream(device);
		LqDustTab tb;
		DBuf d_masked, d_len, d_psum, d_hq, d_q7;
		u64 st[LQSDUST_STATS_WORDS] = {0};
		try {                                                       // (the uploads read the caller's arrays: none stays queued if one throws)
			if (n) {
				d_masked.ensure((size_t)n * 4); d_len.ensure((size_t)n * 4); d_psum.ensure((size_t)n * 8); d_q7.ensure((size_t)n * 4); d_hq.ensure(n);
				LQ_HIP_CHECK(hipMemcpyAsync(d_masked.p, masked, (size_t)n * 4, hipMemcpyHostToDevice, stream));
				LQ_HIP_CHECK(hipMemcpyAsync(d_len.p, len, (size_t)n * 4, hipMemcpyHostToDevice, stream));
				LQ_HIP_CHECK(hipMemcpyAsync(d_psum.p, qual_psum, (size_t)n * 8, hipMemcpyHostToDevice, stream));
				LQ_HIP_CHECK(hipMemcpyAsync(d_q7.p, n_above_q7, (size_t)n * 4, hipMemcpyHostToDevice, stream));
				if (has_q) LQ_HIP_CHECK(hipMemcpyAsync(d_hq.p, has_q, n, hipMemcpyHostToDevice, stream));
				else LQ_HIP_CHECK(hipMemsetAsync(d_hq.p, 0, n, stream));
			}
			const DustTabIn in = {n, d_masked.as<u32>(), d_len.as<u32>(), nullptr, d_psum.as<double>(), d_hq.as<u8>(), nullptr, d_q7.as<u32>()};
			dust_table(tb, stream, in, names, name_off, window, out, out_cap, out_len, st, excl, excl_cap);
		} catch (...) { (void)hipStreamSynchronize(stream); if (stats) memcpy(stats, st, sizeof(st)); throw; }
		if (stats) memcpy(stats, st, sizeof(st));
	});
}

int lqsdust_format(int device, uint32_t n, const char *names, const uint64_t *name_off, const uint32_t *masked, const uint32_t *len,
                   const double *qual_psum, const uint8_t *has_q, const uint32_t *n_above_q7, double window, uint8_t *out, uint64_t out_cap,
                   uint64_t *out_len, lqsdust_stats *stats, char *errbuf, size_t errbuf_len)
{
	return lqsdust_format_lists(device, n, names, name_off, masked, len, qual_psum, has_q, n_above_q7, window, out, out_cap, out_len, stats, nullptr, 0,
	                            errbuf, errbuf_len);
}

} // extern "C"

extern "C" {

int lqsdust_reads(int device, uint32_t n, const uint8_t *seq, const uint64_t *seq_off, const uint8_t *qual, int W, int T,
                  uint32_t *masked, double *qual_psum, uint32_t *n_above_q7, char *errbuf, size_t errbuf_len)
{
	return guarded(errbuf, errbuf_len, [&] {
		if (!seq_off || (n && (!seq || !masked || !qual_psum || !n_above_q7))) throw std::invalid_argument("null buffers");
		select_device(device);
		lqchunk c;
		c.device = device;
		lq_chunk_set(c, n, seq, seq_off, qual);
		lq_chunk_sdust(c, W, T, masked, qual_psum, n_above_q7);
	});
}

// == `sdust [-w W] [-t T] <in.fa>` with stdout -> out_path (sdust.c:181-222)
int lqsdust_main(int argc, const char *const *argv, const char *out_path, const char *err_path, int device)
{
	FILE *e = err_path ? fopen(err_path, "w") : stderr;
	if (!e) return 1;
	int W = 64, T = 20;
	const char *in = nullptr;
	for (int i = 1; i < argc; ++i) {                         // getopt "w:t:" (sdust.c:188-191): -w 64, -w64; first non-option = input
		const char *a = argv[i];
		if (a[0] == '-' && (a[1] == 'w' || a[1] == 't') ) {
			const char *v = a[2] ? a + 2 : (i + 1 < argc ? argv[++i] : nullptr);
			if (!v) { fprintf(e, "sdust: option requires an argument -- '%c'\n", a[1]); if (err_path) fclose(e); return 1; }
			if (a[1] == 'w') W = atoi(v); else T = atoi(v);
		} else if (a[0] == '-' && a[1]) {                      // getopt rejects what "w:t:" does not name
			fprintf(e, "sdust: invalid option -- '%c'\nUsage: sdust [-w %d] [-t %d] <in.fa>\n", a[1], W, T); if (err_path) fclose(e); return 1;
		} else if (!in) in = a;
	}
	if (in && !strcmp(in, "-")) in = "/dev/stdin";            // sdust.c:197: "-" reads standard input
	if (!in) { fprintf(e, "Usage: sdust [-w %d] [-t %d] <in.fa>\n", W, T); if (err_path) fclose(e); return 1; }
	char err[512] = {0};
	int rc = guarded(err, sizeof(err), [&] {
		FILE *t = fopen(in, "rb");
		if (!t) throw lq_open_error(in);
		fclose(t);
		select_device(device);
		FILE *o = out_path ? fopen(out_path, "w") : stdout;
		if (!o) throw lq_open_error(out_path);
		struct Closer { FILE *f; bool own; ~Closer() { if (own && f) fclose(f); else if (f) fflush(f); } } oc{o, out_path != nullptr};
		lqchunk D;                                              // one chunk object for every mini-batch: its buffers grow and stay
		D.device = device;
		FastxReader fr(in);
		std::vector<u32> masked, qv;
		std::vector<double> psum;
		const bool timing = getenv("LQCOV_TIMING") != nullptr;
		const char *split_env = getenv("LQSDUST_SPLIT");          // "pieces": long reads of A/C/G/T alone are cut (kernels_dust_split.hpp); the table is the same
		const bool split = split_env && !strcmp(split_env, "pieces");
		if (split_env && !split && strcmp(split_env, "serial")) throw std::invalid_argument("LQSDUST_SPLIT must be 'serial' or 'pieces'");
		double t_wait = 0, t_dev = 0, t_rows = 0, t_parse = 0;
		// The reader runs ahead on a thread of its own (round 6): mini-batch i + 1 is parsed while mini-batch i is on the device --
		// the two took 0.63 s and 0.64 s one after the other for configs[1]'s 744 Mbases.  Two batches in flight, handed over in order.
		ReadBatch rbs[2];
		std::mutex mu; std::condition_variable cv;
		int filled[2] = {0, 0};                                  // 0: the reader may fill it, 1: ready, 2: the stream is over
		std::exception_ptr rerr;
		std::thread reader([&] {
			try {
				for (int k = 0;; k ^= 1) {
					{ std::unique_lock<std::mutex> lk(mu); cv.wait(lk, [&] { return filled[k] == 0; }); }
					const double ta = lq_now_s();
					rbs[k].clear();
					const bool more = fr.read_minibatch(200000000, rbs[k], true, true) != 0;
					t_parse += lq_now_s() - ta;
					{ std::lock_guard<std::mutex> lk(mu); filled[k] = more ? 1 : 2; }
					cv.notify_all();
					if (!more) break;
				}
			} catch (...) { std::lock_guard<std::mutex> lk(mu); rerr = std::current_exception(); filled[0] = filled[1] = 2; cv.notify_all(); }
		});
		struct Joiner { std::thread &t; std::mutex &mu; std::condition_variable &cv; int *filled; ~Joiner() { { std::lock_guard<std::mutex> lk(mu); if (filled[0] == 1) filled[0] = 0; if (filled[1] == 1) filled[1] = 0; } cv.notify_all(); if (t.joinable()) t.join(); } } joiner{reader, mu, cv, filled};
		double t0 = lq_now_s();
		for (int k = 0;; k ^= 1) {
			{ std::unique_lock<std::mutex> lk(mu); cv.wait(lk, [&] { return filled[k] != 0; }); }
			if (rerr) std::rethrow_exception(rerr);
			if (filled[k] == 2) break;
			ReadBatch &rb = rbs[k];
			const u32 n = rb.size();
			masked.resize(n); qv.resize(n); psum.resize(n);
			double t1 = lq_now_s(); t_wait += t1 - t0;
			lq_chunk_set(D, n, rb.seq.data(), rb.seq_off.data(), rb.any_qual ? rb.qual.data() : nullptr);
			if (split) lq_chunk_sdust_split(D, W, T, 0, masked.data(), psum.data(), qv.data(), nullptr);
			else lq_chunk_sdust(D, W, T, masked.data(), psum.data(), qv.data());
			t0 = lq_now_s(); t_dev += t0 - t1;
			dust_print_rows(o, rb, masked.data(), psum.data(), qv.data());
			t1 = lq_now_s(); t_rows += t1 - t0; t0 = t1;
			{ std::lock_guard<std::mutex> lk(mu); filled[k] = 0; }
			cv.notify_all();
		}
		if (timing) fprintf(e, "[timing] sdust: parse %.3f s on the reader's thread (waited for: %.3f s), upload + kernel + download %.3f s, rows %.3f s\n", t_parse, t_wait, t_dev, t_rows);
	});
	if (rc) fprintf(e, "ERROR: %s\n", err);
	if (err_path) fclose(e);
	return rc == 0 ? 0 : (rc == LQCOV_E_IO ? 1 : rc);
}

} // extern "C"
