// longqc_amd/csrc/kernels_gzip.hpp -- a plain gzip stream inflated on the device by speculative spans (gzip.hpp drives it; the
// two-pass scheme of pugz and rapidgzip, written from its description).  A gzip member that is not BGZF says nowhere how long its
// deflate blocks are, so the uploaded compressed window is cut into spans of span_bytes and
//   k_gz_find          looks in every span for the first bit offset at which a non-final dynamic-Huffman block header parses
//                      completely: lanes test 64 consecutive offsets with the field tests (BFINAL 0, BTYPE 2, HLIT and HDIST <= 29, a
//                      complete code-length code), the survivors go, in offset order and wave-uniformly, through the header parse the
//                      decoder itself uses.  No such offset: the span is empty and its bytes belong to the span before it.  Stored and
//                      fixed-code blocks are not searched for;
//   k_gz_inflate_spec  decodes every non-empty span from its start without knowing the 32 KiB in front of it: the output is 16-bit
//                      symbols, below 256 a byte, 256 + i "byte i of the 32 KiB in front of this span".  One wave per span, the sliding
//                      history a ring of 32 Ki symbols in LDS (64 KiB, with the tables two workgroups per CU as k_bgzf_inflate), the
//                      symbols stream out to the span's region in aligned 16-byte words.  A span ends at the first block boundary at or
//                      behind the next non-empty span's start, behind a final block, or at the last boundary that fitted its region;
//   k_gz_window        runs over the accepted spans one after another and makes the 32-KiB window behind each from the window in front
//                      of it and the span's last symbols;
//   k_gz_resolve       all accepted spans side by side: every symbol becomes its byte, at the span's place in the destination.
// Whether a span's start was a block boundary at all is the host's to say (the chain: span i + 1 counts only if it starts where
// span i ended), and what a kernel reports as wrong the host has zlib decide.  For any input every kernel reads only the aligned
// words that hold the window and its own symbols, writes only inside the span's region / the span's bytes of the destination, and
// ends: every loop iteration consumes input or fails.
#pragma once
#include "kernels_inflate.hpp"

#define LQ_GZ_THREADS 64
#define LQ_GZ_MAX_BLOCKS 512u        // spans are strided over the workgroups of a launch: two per CU
#define LQ_GZ_MAX_SPANS 2048u        // spans of one window
#define LQ_GZ_WIN 32768u             // the deflate history
#define LQ_GZ_NONE 0xffffffffu       // an empty span's start; no stop
#define LQ_GZ_FLUSH 16384u           // symbols in the ring that are not in global memory yet: at most this many and one token / copy step
#define LQ_GZ_WINDOW_THREADS 1024
#define LQ_GZ_RESOLVE_THREADS 256

enum { LQ_GZ_OK = 0, LQ_GZ_INVALID = 1, LQ_GZ_INPUT = 2, LQ_GZ_FULL = 3 };

// one span to decode: from bit start_bit of the window to the first block boundary at or behind stop_bit; its symbols go to
// syms[sym_off .. sym_off + cap) (sym_off, cap: multiples of 8); hist: the bytes of the member known to lie in front of it
// (LQ_GZ_NONE: unknown, at least 32 KiB as far as the kernel can tell)
struct alignas(8) GzJob { u64 sym_off; u32 start_bit, stop_bit, cap, hist; };
// what came of it: [start_bit, end_bit) whole blocks that gave n_out symbols; status: why it stopped there (LQ_GZ_OK: at its stop or
// behind a final block)
struct GzSpan { u32 start_bit, end_bit, n_out, status, saw_final; };
// an accepted span: n_out symbols at syms[sym_off ..) become out[out_off ..); hist: bytes of the member in front of it, at most 32768
struct alignas(8) GzAcc { u64 sym_off, out_off; u32 n_out, hist; };

struct LqGzTabs { u16 *tab_l, *tab_d, *order_l, *order_d, *cnt_l, *cnt_d; u8 *lens, *cl19; };

__device__ __forceinline__ void lq_gz_bits(LqBits &b, const u8 *comp, u32 comp_len, u32 bit)
{
	b.a0 = 0; b.words = (const u32*)comp; b.n_words = (comp_len + 3) >> 2; b.total = comp_len * 8;
	lq_inf_seek(b, bit >> 3);
	lq_inf_take(b, bit & 7);
}

// the header of a dynamic block behind its three first bits, and both decode tables -> 0 or LQ_GZ_*.  Wave-collective.
__device__ __forceinline__ u32 lq_gz_dynamic(LqBits &b, const LqGzTabs &t)
{
	const u32 lane = threadIdx.x & 63;
	lq_inf_refill(b);
	const u32 nlen = lq_inf_take(b, 5) + 257, ndist = lq_inf_take(b, 5) + 1, ncode = lq_inf_take(b, 4) + 4;
	if (b.used > b.total) return LQ_GZ_INPUT;
	if (nlen > 286 || ndist > 30) return LQ_GZ_INVALID;
	__syncthreads();                                          // (nobody reads the lengths of the block before)
	if (lane < 19) t.cl19[lane] = 0;
	__syncthreads();
	for (u32 i = 0; i < ncode; ++i) {
		lq_inf_refill(b);
		const u32 l = lq_inf_take(b, 3);
		if (lane == 0) t.cl19[lq_inf_order19[i]] = (u8)l;
	}
	if (b.used > b.total) return LQ_GZ_INPUT;
	if (lq_inf_build(t.cl19, 19, 7, true, t.tab_l, t.order_l, t.cnt_l)) return LQ_GZ_INVALID;
	u32 i = 0, prev = 0;                                      // the lengths of both alphabets are one run
	while (i < nlen + ndist) {
		lq_inf_refill(b);
		u32 cl;
		const u32 sym = lq_inf_symbol(b, 7, t.tab_l, t.order_l, t.cnt_l, &cl);
		if (sym == 0xffff) return b.total - b.used < 7 ? LQ_GZ_INPUT : LQ_GZ_INVALID;
		lq_inf_take(b, cl);
		u32 rep = 1, val = sym;
		if (sym == 16) { if (i == 0) return LQ_GZ_INVALID; val = prev; rep = 3 + lq_inf_take(b, 2); }
		else if (sym == 17) { val = 0; rep = 3 + lq_inf_take(b, 3); }
		else if (sym == 18) { val = 0; rep = 11 + lq_inf_take(b, 7); }
		if (b.used > b.total) return LQ_GZ_INPUT;
		if (i + rep > nlen + ndist) return LQ_GZ_INVALID;
		if (lane == 0) for (u32 r = 0; r < rep; ++r) t.lens[i + r] = (u8)val;
		i += rep; prev = val;
	}
	__syncthreads();
	if (t.lens[256] == 0) return LQ_GZ_INVALID;               // no end-of-block code
	if (lq_inf_build(t.lens, nlen, LQ_INF_FAST, false, t.tab_l, t.order_l, t.cnt_l)) return LQ_GZ_INVALID;
	if (lq_inf_build(t.lens + nlen, ndist, LQ_INF_FAST, false, t.tab_d, t.order_d, t.cnt_d)) return LQ_GZ_INVALID;
	return 0;
}

// n <= 25 bits of the window from bit `bit` on (zeros behind the last word)
__device__ __forceinline__ u32 lq_gz_peek(const u32 *w, u32 n_words, u32 bit, u32 n)
{
	const u32 k = bit >> 5;
	const u64 x = (u64)(k < n_words ? w[k] : 0u) | (u64)(k + 1 < n_words ? w[k + 1] : 0u) << 32;
	return (u32)(x >> (bit & 31)) & ((1u << n) - 1);
}

// the field tests of one bit offset: BFINAL 0, BTYPE 2, HLIT <= 29, HDIST <= 29, the lengths of the code-length code a complete
// code (Kraft sum exactly one), all of it in front of bit `hi`
__device__ __forceinline__ bool lq_gz_cheap(const u32 *w, u32 n_words, u32 bit, u32 hi)
{
	if (bit + 17 > hi) return false;
	const u32 h = lq_gz_peek(w, n_words, bit, 17);
	if ((h & 7) != 4 || (h >> 3 & 31) > 29 || (h >> 8 & 31) > 29) return false;
	const u32 ncode = (h >> 13) + 4;
	if (bit + 17 + 3 * ncode > hi) return false;
	u32 sum = 0;
	for (u32 i = 0; i < ncode; i += 7) {
		u32 v = lq_gz_peek(w, n_words, bit + 17 + 3 * i, 21);
		const u32 m = ncode - i < 7 ? ncode - i : 7;
		for (u32 j = 0; j < m; ++j, v >>= 3) if (v & 7) sum += 128u >> (v & 7);
	}
	return sum == 128;
}

// start_bit[s], s = 1 .. n_spans - 1: the first bit offset in span s = bytes [s * span_bytes, (s + 1) * span_bytes) of the window at
// which a non-final dynamic block's header parses completely inside the span, LQ_GZ_NONE if there is none.  (Span 0 starts where the
// host says.)  comp: 4-byte aligned, LQ_INFLATE_PAD bytes allocated past the last; comp_len < 2^28
__global__ void __launch_bounds__(LQ_GZ_THREADS)
k_gz_find(const u8 *comp, u32 comp_len, u32 span_bytes, u32 n_spans, u32 *start_bit)
{
	__shared__ u16 tab_l[1 << LQ_INF_FAST], tab_d[1 << LQ_INF_FAST];
	__shared__ u16 order_l[288], order_d[32], cnt_l[16], cnt_d[16];
	__shared__ u8 lens[320], cl19[32];
	const LqGzTabs t = {tab_l, tab_d, order_l, order_d, cnt_l, cnt_d, lens, cl19};
	const u32 lane = threadIdx.x & 63;
	const u32 *w = (const u32*)comp; const u32 n_words = (comp_len + 3) >> 2;
	for (u32 s = 1 + blockIdx.x; s < n_spans; s += gridDim.x) {
		const u64 lo64 = (u64)s * span_bytes, hi64 = lo64 + span_bytes;
		const u32 lo = (u32)(lo64 < comp_len ? lo64 : comp_len) * 8, hi = (u32)(hi64 < comp_len ? hi64 : comp_len) * 8;
		u32 found = LQ_GZ_NONE;
		for (u32 o = lo; o < hi && found == LQ_GZ_NONE; o += 64) {
			u64 m = __ballot(lq_gz_cheap(w, n_words, o + lane, hi));
			while (m) {                                           // the survivors, in offset order: the decoder's own header parse
				const u32 cand = o + (u32)__ffsll((unsigned long long)m) - 1;
				m &= m - 1;
				LqBits b;
				lq_gz_bits(b, comp, comp_len, cand);
				lq_inf_refill(b);
				lq_inf_take(b, 3);
				if (lq_gz_dynamic(b, t) == 0 && b.used <= hi) { found = cand; break; }
			}
		}
		if (lane == 0) start_bit[s] = found;
	}
}

// ring[flushed .. upto & ~7) -> dst, in words of eight symbols (flushed is a multiple of 8, so is the ring's length)
__device__ __forceinline__ void lq_gz_flush(const u16 *ring, u16 *dst, u32 &flushed, u32 upto)
{
	__syncthreads();                                          // the symbols stored so far, by whichever lane, are there
	const u32 end = upto & ~7u;
	for (u32 i = flushed + (threadIdx.x & 63) * 8; i < end; i += 64 * 8) *(uint4*)(dst + i) = *(const uint4*)(ring + (i & (LQ_GZ_WIN - 1)));
	if (end > flushed) flushed = end;
	__syncthreads();                                          // every lane has read its words: the slots may be stored to again
}

// n_jobs spans: syms: 16-byte aligned; spans[j]: what came of job j
__global__ void __launch_bounds__(LQ_GZ_THREADS)
k_gz_inflate_spec(const u8 *comp, u32 comp_len, const GzJob *jobs, u32 n_jobs, u16 *syms, GzSpan *spans)
{
	__shared__ uint4 ring4[LQ_GZ_WIN / 8];                    // the last 32 Ki symbols
	__shared__ u16 tab_l[1 << LQ_INF_FAST], tab_d[1 << LQ_INF_FAST];
	__shared__ u16 order_l[288], order_d[32], cnt_l[16], cnt_d[16];
	__shared__ u8 lens[320], cl19[32];
	const LqGzTabs t = {tab_l, tab_d, order_l, order_d, cnt_l, cnt_d, lens, cl19};
	u16 *ring = (u16*)ring4;
	const u32 lane = threadIdx.x & 63, RM = LQ_GZ_WIN - 1;
	for (u32 j = blockIdx.x; j < n_jobs; j += gridDim.x) {
		const GzJob job = jobs[j];
		u16 *dst = syms + job.sym_off;
		LqBits b;
		lq_gz_bits(b, comp, comp_len, job.start_bit);
		u32 pos = 0, flushed = 0, st = LQ_GZ_OK;
		u32 end_bit = job.start_bit, n_out = 0, fin = 0;          // the last block boundary
		for (;;) {
			lq_inf_refill(b);
			const u32 last = lq_inf_take(b, 1), type = lq_inf_take(b, 2);
			if (b.used > b.total) { st = LQ_GZ_INPUT; break; }
			if (type == 3) { st = LQ_GZ_INVALID; break; }
			if (type == 0) {                                          // stored: LEN, ~LEN at the next byte border, then the bytes
				const u32 at = (b.used + 7) >> 3;
				if (at + 4 > comp_len) { st = LQ_GZ_INPUT; break; }
				lq_inf_seek(b, at);
				lq_inf_refill(b);
				const u32 v = lq_inf_take(b, 32), n = v & 0xffff;
				if ((v >> 16) != (n ^ 0xffff)) { st = LQ_GZ_INVALID; break; }
				if (n > comp_len - (at + 4)) { st = LQ_GZ_INPUT; break; }
				if (n > job.cap - pos) { st = LQ_GZ_FULL; break; }
				const u8 *src = comp + at + 4;
				for (u32 done = 0; done < n;) {
					const u32 m = n - done < 8192 ? n - done : 8192u;
					for (u32 i = lane; i < m; i += 64) ring[(pos + i) & RM] = src[done + i];
					pos += m; done += m;
					if (pos - flushed >= LQ_GZ_FLUSH) lq_gz_flush(ring, dst, flushed, pos);
				}
				lq_inf_seek(b, at + 4 + n);
			} else {
				if (type == 1) {                                      // the fixed codes (RFC 1951 3.2.6)
					__syncthreads();
					for (u32 i = lane; i < 320; i += 64) lens[i] = i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : i < 288 ? 8 : 5;
					lq_inf_build(lens, 288, LQ_INF_FAST, false, tab_l, order_l, cnt_l);
					lq_inf_build(lens + 288, 32, LQ_INF_FAST, false, tab_d, order_d, cnt_d);
				} else if ((st = lq_gz_dynamic(b, t)) != 0) break;
				for (;;) {                                            // the block's symbols
					lq_inf_refill(b);
					u32 cl;
					u32 sym = lq_inf_symbol(b, LQ_INF_FAST, tab_l, order_l, cnt_l, &cl);
					if (sym == 0xffff) { st = b.total - b.used < 15 ? LQ_GZ_INPUT : LQ_GZ_INVALID; break; }
					lq_inf_take(b, cl);
					if (b.used > b.total) { st = LQ_GZ_INPUT; break; }
					if (sym < 256) {
						if (pos >= job.cap) { st = LQ_GZ_FULL; break; }
						if (lane == 0) ring[pos & RM] = (u16)sym;
						++pos;
					} else {
						if (sym == 256) break;
						if (sym > 285) { st = LQ_GZ_INVALID; break; }
						sym -= 257;
						const u32 lx = sym < 8 || sym == 28 ? 0u : (sym - 4) >> 2;
						const u32 len = (sym < 8 ? sym + 3 : sym == 28 ? 258u : ((4 + (sym & 3)) << lx) + 3) + lq_inf_take(b, lx);
						if (b.used > b.total) { st = LQ_GZ_INPUT; break; }
						lq_inf_refill(b);
						const u32 ds = lq_inf_symbol(b, LQ_INF_FAST, tab_d, order_d, cnt_d, &cl);
						if (ds == 0xffff) { st = b.total - b.used < 15 ? LQ_GZ_INPUT : LQ_GZ_INVALID; break; }
						lq_inf_take(b, cl);
						if (b.used > b.total) { st = LQ_GZ_INPUT; break; }
						if (ds > 29) { st = LQ_GZ_INVALID; break; }
						const u32 dx = ds < 4 ? 0u : (ds - 2) >> 1;
						const u32 dist = (ds < 4 ? ds + 1 : ((2 + (ds & 1)) << dx) + 1) + lq_inf_take(b, dx);
						if (b.used > b.total) { st = LQ_GZ_INPUT; break; }
						if (job.hist != LQ_GZ_NONE && dist > pos && dist - pos > job.hist) { st = LQ_GZ_INVALID; break; }      // in front of the member
						if (len > job.cap - pos) { st = LQ_GZ_FULL; break; }
						// symbol pos + i is symbol pos - dist + i % dist; one in front of the span is a marker: 256 + its place in the
						// 32 KiB there.  A distance within a copy's length of the ring's: a lane's slot is another lane's source
						// (slot pos + i holds symbol pos + i - 32768), so every 64 are read before they are stored
						const i32 s0 = (i32)pos - (i32)dist;
						__syncthreads();                                  // the symbols stored so far, by whichever lane, are there
						if (dist > LQ_GZ_WIN - 258) {
							for (u32 base = 0; base < len; base += 64) {
								const u32 i = base + lane;
								const i32 s = s0 + (i32)(i % dist);
								const u16 v = i >= len ? (u16)0 : s < 0 ? (u16)(256 + (i32)LQ_GZ_WIN + s) : ring[(u32)s & RM];
								__syncthreads();
								if (i < len) ring[(pos + i) & RM] = v;
								__syncthreads();
							}
						} else {
							for (u32 i = lane; i < len; i += 64) {
								const i32 s = s0 + (i32)(dist >= len ? i : i % dist);
								ring[(pos + i) & RM] = s < 0 ? (u16)(256 + (i32)LQ_GZ_WIN + s) : ring[(u32)s & RM];
							}
						}
						pos += len;
					}
					if (pos - flushed >= LQ_GZ_FLUSH) lq_gz_flush(ring, dst, flushed, pos);
				}
				if (st) break;
			}
			end_bit = b.used; n_out = pos; fin = last;                // a block boundary
			if (last || b.used >= job.stop_bit) break;
		}
		// what the ring still holds of the whole blocks: words, then the symbols behind the last whole word
		if (n_out > flushed) {
			lq_gz_flush(ring, dst, flushed, n_out);
			if (lane < n_out - flushed) dst[flushed + lane] = ring[(flushed + lane) & RM];
		}
		if (lane == 0) { GzSpan r; r.start_bit = job.start_bit; r.end_bit = end_bit; r.n_out = n_out; r.status = st; r.saw_final = fin; spans[j] = r; }
		__syncthreads();                                          // the ring is free for the next span
	}
}

// wins: (n + 1) windows of 32 KiB; wins[0]: the 32 KiB in front of the first accepted span (its last acc[0].hist bytes are the
// member's), wins[k + 1]: the 32 KiB behind span k.  One workgroup, span after span.  status[k] = 1: a marker of span k points in
// front of the member's first byte
__global__ void __launch_bounds__(LQ_GZ_WINDOW_THREADS)
k_gz_window(const u16 *syms, const GzAcc *acc, u32 n, u8 *wins, u32 *status)
{
	for (u32 k = 0; k < n; ++k) {
		const GzAcc a = acc[k];
		const u8 *w = wins + (u64)k * LQ_GZ_WIN; u8 *o = wins + (u64)(k + 1) * LQ_GZ_WIN;
		const u16 *s = syms + a.sym_off;
		bool bad = false;
		for (u32 j = threadIdx.x; j < LQ_GZ_WIN; j += blockDim.x) {       // byte j of the last 32 KiB of (window, span)
			const u64 p = (u64)a.n_out + j;
			u32 v;
			if (p < LQ_GZ_WIN) v = w[p];
			else {
				v = s[p - LQ_GZ_WIN];
				if (v >= 256) { v -= 256; if (LQ_GZ_WIN - v > a.hist) bad = true; v = w[v]; }
			}
			o[j] = (u8)v;
		}
		if (bad) status[k] = 1;
		__syncthreads();                                          // the next span reads what this one wrote
	}
}

// every symbol of the accepted spans becomes its byte at out[out_off ..): aligned 16-byte words, single bytes in front of the first
// and behind the last whole word.  *markers: how many symbols were markers
__global__ void __launch_bounds__(LQ_GZ_RESOLVE_THREADS)
k_gz_resolve(const u16 *syms, const GzAcc *acc, u32 n, const u8 *wins, u8 *out, u32 *status, unsigned long long *markers)
{
	for (u32 k = blockIdx.x; k < n; k += gridDim.x) {
		const GzAcc a = acc[k];
		const u8 *w = wins + (u64)k * LQ_GZ_WIN;
		const u16 *s = syms + a.sym_off;
		u8 *d = out + a.out_off;
		u32 cnt = 0; bool bad = false;
		auto byte = [&](u32 i) -> u32 {
			u32 v = s[i];
			if (v >= 256) { v -= 256; ++cnt; if (LQ_GZ_WIN - v > a.hist) bad = true; v = w[v]; }
			return v;
		};
		const u32 to16 = (u32)((16 - ((u64)(uintptr_t)d & 15)) & 15);
		const u32 head = a.n_out < to16 ? a.n_out : to16, body = (a.n_out - head) & ~15u, tail = a.n_out - head - body;
		if (threadIdx.x < head) d[threadIdx.x] = (u8)byte(threadIdx.x);
		for (u32 i = threadIdx.x * 16; i < body; i += LQ_GZ_RESOLVE_THREADS * 16) {
			u32 q[4];
			for (u32 c = 0; c < 4; ++c) {
				const u32 at = head + i + 4 * c;
				q[c] = byte(at) | byte(at + 1) << 8 | byte(at + 2) << 16 | byte(at + 3) << 24;
			}
			uint4 v; v.x = q[0]; v.y = q[1]; v.z = q[2]; v.w = q[3];
			*(uint4*)(d + head + i) = v;
		}
		if (threadIdx.x < tail) d[head + body + threadIdx.x] = (u8)byte(head + body + threadIdx.x);
		if (bad) status[k] = 1;
		if (cnt) atomicAdd(markers, (unsigned long long)cnt);
	}
}
