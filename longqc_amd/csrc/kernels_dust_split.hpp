// longqc_amd/csrc/kernels_dust_split.hpp -- the low-complexity scan in pieces: several threads per long read, opt-in
// beside k_sdust (kernels_dust.hpp), which stays as it is and keeps every read this mode cannot serve.
//
// What the pieces rest on (sdust.c:72-166; checked against the reference binary by tools/fuzz_sdust_split.py):
//   1. The state of sdust_core before step b is a function of the triplet words pushed shortly before b: W - 2 pushes make the
//      window, its counts and the suffix L exact, the next W steps every perfect interval that can still be alive at b.  A scan that
//      starts from empty state 2 W pushes -- 2 W + 2 bases, the first two push nothing -- before b and keeps only what it saves at
//      steps >= b saves what the serial scan saves there.
//   2. In a read of A/C/G/T alone the saves come in ascending start order and none passes the read's end, so the reference's merged
//      total (sdust.c:94-108, 208-209) is the number of bases in the union of the saved intervals: a bit mask, one bit per base,
//      filled by atomicOr in any order.
//   3. Any other byte clears P but keeps the window (sdust.c:158-161); later saves can then start before earlier ones and the merged
//      total is a fold over the save order, not a union.  Such reads, and reads too short to cut, are flagged and walked by k_sdust.
//
//   k_sdust_classify    flag[r] = 1 for a read with a byte k_sdust does not take for A/C/G/T (either case) or with fewer than
//                       min_len bases.  Byte-parallel: a wave takes an aligned tile of 4096 bytes of the chunk (4 x 16-byte loads per
//                       lane, as k_gc_reads) and visits the reads that overlap it.
//   k_sdust_pieces      one thread per (read, piece) item of the unflagged reads, k_sdust's LDS layout and DustPI ring; the thread
//                       starts LQ_DUST_SPLIT_HALO(W) bases before its piece and ORs what it saves at its own steps into the mask
//   k_sdust_mask_count  masked[r] = set bits of read r's part of the mask, a wave per unflagged read
//   k_sdust_qual        the two quality columns, one thread per read (the double sum is sequential by contract, lqutils.c:51-56)
//   k_sdust_compact / k_sdust_scatter   the flagged reads' bases into a buffer of their own for k_sdust, and its counts back
// The mask is over the chunk's concatenated bases: bit off[r] + j is base j of read r (bit g = bit g & 31 of word g >> 5).
#pragma once
#include "kernels_dust.hpp"

#define LQ_DUST_SPLIT_PIECE 4096u           // bases per piece unless the caller says otherwise
#define LQ_DUST_SPLIT_MIN_PIECES 2          // LQ_DUST_SPLIT_MIN: a read of fewer than this many pieces' bases takes the serial walk
#define LQ_DUST_SPLIT_MAX_THREADS 131072    // (read, piece) items per launch; the others are strided over them
#define LQ_DUST_SPLIT_TILE 4096u            // k_sdust_classify: bytes of one (wave, tile) = LQ_CHUNK_SEQ_TILE
#define LQ_DUST_SPLIT_THREADS 256           // k_sdust_classify, k_sdust_mask_count, k_sdust_compact, k_sdust_scatter
#define LQ_DUST_SPLIT_MAX_BLOCKS 2048       // ... and their grid cap: tiles / reads are strided over the launch
#ifndef LQ_DUST_SPLIT_HALO
#define LQ_DUST_SPLIT_HALO(W) (2 * (W) + 2)    // bases walked before a piece from empty state (fact 1); also the smallest piece
#endif
#define LQ_DUST_SPLIT_MIN(piece) ((u64)LQ_DUST_SPLIT_MIN_PIECES * (piece))

// the last r in [0, n] with off[r] <= x (off ascending, off[0] <= x): the read that holds byte / item x, empty ones skipped (lq_gc_find)
__device__ __forceinline__ u32 lq_dust_find(const u64 *off, u32 n, u64 x)
{
	u32 lo = 0, hi = n;                                       // invariant: off[lo] <= x, and off[hi + 1] > x or hi == n
	while (lo < hi) {
		const u32 mid = lo + (hi - lo + 1) / 2;
		if (off[mid] <= x) lo = mid; else hi = mid - 1;
	}
	return lo;
}

// 0x80 in every byte of x that is none of A, C, G, T in either case (k_sdust's `ch & 0xdf` and its four comparisons)
__device__ __forceinline__ u32 lq_dust_other(u32 x)
{
	const u32 u = x & 0xdfdfdfdfu;
	const u32 a = u ^ 0x41414141u, cg = (u & 0xfbfbfbfbu) ^ 0x43434343u, t = u ^ 0x54545454u;      // a zero byte where u had A / C or G / T
#define LQ_DUST_ZB(y) (~((((y) & 0x7f7f7f7fu) + 0x7f7f7f7fu) | (y) | 0x7f7f7f7fu))
	const u32 ok = LQ_DUST_ZB(a) | LQ_DUST_ZB(cg) | LQ_DUST_ZB(t);
#undef LQ_DUST_ZB
	return ~ok & 0x80808080u;
}

// the same as four bits: bit k for byte k
__device__ __forceinline__ u32 lq_dust_other4(u32 x)
{
	const u32 y = lq_dust_other(x) >> 7;
	return (y | y >> 7 | y >> 14 | y >> 21) & 0xfu;
}

// buf: the chunk's bases, allocated in whole tiles; off[0..n]: the reads' offsets; flag[0..n): zero on entry
__global__ void __launch_bounds__(LQ_DUST_SPLIT_THREADS)
k_sdust_classify(const u8 *buf, const u64 *off, u32 n, u64 min_len, u8 *flag)
{
	for (u64 r = (u64)blockIdx.x * LQ_DUST_SPLIT_THREADS + threadIdx.x; r < n; r += (u64)gridDim.x * LQ_DUST_SPLIT_THREADS)
		if (off[r + 1] - off[r] < min_len) flag[r] = 1;
	const u32 lane = threadIdx.x & 63;
	const u64 total = off[n], n_tiles = (total + LQ_DUST_SPLIT_TILE - 1) / LQ_DUST_SPLIT_TILE;
	const u64 wave = (u64)blockIdx.x * (LQ_DUST_SPLIT_THREADS / 64) + threadIdx.x / 64, n_waves = (u64)gridDim.x * (LQ_DUST_SPLIT_THREADS / 64);
	for (u64 t = wave; t < n_tiles; t += n_waves) {
		const u64 A = t * LQ_DUST_SPLIT_TILE, Aend = A + LQ_DUST_SPLIT_TILE < total ? A + LQ_DUST_SPLIT_TILE : total;
		const uint4 *src = (const uint4*)(buf + A);
		u64 bad = 0;                                             // bit 16 i + k: byte k of this lane's load i is another byte
		for (int i = 0; i < 4; ++i) {
			const uint4 v = src[i * 64 + lane];
			bad |= (u64)(lq_dust_other4(v.x) | lq_dust_other4(v.y) << 4 | lq_dust_other4(v.z) << 8 | lq_dust_other4(v.w) << 12) << (16 * i);
		}
		for (u32 r = lq_dust_find(off, n, A); r < n; ++r) {          // (wave-uniform: every lane walks the same reads)
			const u64 lo = off[r], hi = off[r + 1];
			if (lo >= Aend) break;
			if (hi == lo) continue;
			const u32 m_lo = lo > A ? (u32)(lo - A) : 0u, m_hi = (u32)((hi < Aend ? hi : Aend) - A);      // offsets in the tile
			u32 c = 0;
			for (int i = 0; i < 4; ++i) {
				const u32 a = (u32)(i * 64 + lane) * 16;           // the load's offset in the tile: its bytes [s, e) lie in the read
				const u32 s = m_lo > a ? (m_lo - a < 16 ? m_lo - a : 16u) : 0u, e = m_hi > a ? (m_hi - a < 16 ? m_hi - a : 16u) : 0u;
				if (e > s) c |= (u32)(bad >> (16 * i)) & 0xffffu & (0xffffu << s) & (0xffffu >> (16 - e));
			}
			c = c != 0;
			for (int d = 32; d; d >>= 1) c |= __shfl_xor(c, d);
			if (lane == 0 && c) flag[r] = 1;                       // (every writer writes 1)
		}
	}
}

// set bits [g0, g1) of the mask (bit numbers of 32 bits: the host refuses a chunk of 2^32 bases), word by word with atomicOr: other pieces
// and the neighbouring reads write the same words.  Not inlined: a run of saves closes rarely, and the copies inside k_sdust_pieces'
// loop cost that kernel registers (51 against k_sdust's 49; 48 with the call)
__device__ __noinline__ void lq_dust_mask_or(u32 *mask, u32 g0, u32 g1)
{
	if ((i32)(g1 - g0) <= 0) return;
	const u32 w0 = g0 >> 5, w1 = (g1 - 1) >> 5;
	const u32 m0 = ~0u << (g0 & 31), m1 = ~0u >> (31 - ((g1 - 1) & 31));
	if (w0 == w1) { atomicOr(mask + w0, m0 & m1); return; }
	atomicOr(mask + w0, m0);
	for (u32 w = w0 + 1; w < w1; ++w) atomicOr(mask + w, ~0u);
	atomicOr(mask + w1, m1);
}

// item_off[0..n_reads]: (read, piece) items before read r (a flagged read has none; fewer than 2^31 in all); item it of read r is bases
// [p * piece, (p + 1) * piece) with p = it - item_off[r], cut at the read's end, and the last piece owns the end-of-read step.  The state machine is
// k_sdust's; what differs is where it starts, that positions count from the piece's first base, that a save counts only from there on, and
// that the merged saves go to the mask
__global__ void __launch_bounds__(LQ_DUST_THREADS)
k_sdust_pieces(const u8 *seq, const u64 *seq_off, const u64 *item_off, u32 n_reads, u32 n_items, u32 piece, i32 W, i32 T,
               DustPI *pi_scratch, u32 *mask)
{
	LQ_SHARED u8 s_q[64][LQ_DUST_THREADS], s_cw[64][LQ_DUST_THREADS], s_cv[64][LQ_DUST_THREADS], s_c[64][LQ_DUST_THREADS];
	const u32 tid = blockIdx.x * blockDim.x + threadIdx.x, n_threads = gridDim.x * blockDim.x;
	const u32 ln = threadIdx.x;
	DustPI *P = pi_scratch + (u64)tid * LQ_DUST_PCAP;
	const i32 halo = LQ_DUST_SPLIT_HALO(W);
	// positions are counted from the piece's first base (the halo's are negative): what decides a save is the sign of the step
	for (u32 it = tid; it < n_items; it += n_threads) {
	const u32 r = lq_dust_find(item_off, n_reads, it);
	const u64 pb = (u64)(it - (u32)item_off[r]) * piece;          // the piece's first base in the read (< len <= 2^31 - 1)
	const u8 *s = seq + seq_off[r] + pb;
	const i32 len = (i32)(seq_off[r + 1] - seq_off[r] - pb);      // the read's end
	const i32 i_begin = pb > (u64)halo ? -halo : -(i32)pb, i_end = len > (i32)piece ? (i32)piece : len + 1;
	for (int i = 0; i < 64; ++i) { s_cw[i][ln] = 0; s_cv[i][ln] = 0; }
	i32 qn = 0, qh = 0, rw = 0, rv = 0, L = 0;
	u64 occ = 0;                                               // non-empty buckets (bit = start & 63)
	i32 pmin = 0, pmax = 0;                                    // smallest / largest live start (occ != 0)
	i32 l = 0, ls = 0, lf = -0x7fffffff;                       // [ls, lf): the run of saves not yet in the mask; none: it ends before every start
	u32 t = 0;
	// LQ_DUST_FLUSH of k_sdust; the interval is saved only at the piece's own steps, and a closed run of saves goes to the mask.  An
	// interval made at step i ends at base i + 1 (finish = start + qn + 2) and starts at or after the scan's first base: inside the read
#define LQ_DUST_SPLIT_FLUSH(start_) do { \
		const i32 st_ = (start_); \
		if (occ != 0 && pmin < st_) { \
			if (i >= 0) { \
				const i32 p_start_ = pmin, p_fin_ = P[pmin & 63].finish; \
				if (p_start_ <= lf) { if (p_fin_ > lf) lf = p_fin_; } \
				else { lq_dust_mask_or(mask, (u32)(s - seq) + (u32)ls, (u32)(s - seq) + (u32)lf); ls = p_start_; lf = p_fin_; } \
			} \
			for (i32 s_ = pmin; s_ < st_ && s_ <= pmax; ++s_) occ &= ~(1ULL << (s_ & 63)); \
			if (occ != 0) { i32 s_ = st_; while (!(occ >> (s_ & 63) & 1)) ++s_; pmin = s_; } \
		} \
	} while (0)
	for (i32 i = i_begin; i < i_end; ++i) {
		const u32 ch = i < len ? s[i] : 0u;
		const u32 cu = ch & 0xdfu;                             // upper case
		const i32 b = cu == 'A' ? 0 : cu == 'C' ? 1 : cu == 'G' ? 2 : cu == 'T' ? 3 : -1;   // seq_nt4_table of sdust.c:25-42
		// (one flush site for both kinds of step: every copy of it costs registers)
		i32 start;
		if (b >= 0) {
			++l; t = (t << 2 | (u32)b) & 63u;
			if (l < 3) continue;
			start = (l - W > 0 ? l - W : 0) + (i + 1 - l);
		} else start = (l - W + 1 > 0 ? l - W + 1 : 0) + (i + 1 - l);
		for (;;) {                                             // a word: once; the end of the read: `while (occ) { flush; ++start; }`
			LQ_DUST_SPLIT_FLUSH(start);
			if (b >= 0 || !occ) break;
			++start;
		}
		if (b < 0) { l = 0; t = 0; continue; }                 // (an unflagged read holds no other byte: this was the end-of-read step)
		{
			{
				// shift_window (sdust.c:70-91)
				if (qn >= W - 3 + 1) {
					const u32 so = s_q[qh][ln]; qh = (qh + 1) & 63; --qn;
					rw -= --s_cw[so][ln];
					if (L > qn) { --L; rv -= --s_cv[so][ln]; }
				}
				s_q[(qh + qn) & 63][ln] = (u8)t; ++qn;
				++L;
				rw += s_cw[t][ln]++;
				rv += s_cv[t][ln]++;
				if ((i32)s_cv[t][ln] * 10 > T << 1) {
					u32 so;
					do {
						so = s_q[(qh + qn - L) & 63][ln];
						rv -= --s_cv[so][ln];
						--L;
					} while (so != t);
				}
				if (rw * 10 > L * T) {
					// find_perfect (sdust.c:110-134)
					for (int z = 0; z < 64; ++z) s_c[z][ln] = s_cv[z][ln];
					i32 rr = rv, max_r = 0, max_l = 0;
					i32 folded = occ ? pmax + 1 : 0;               // buckets with start >= folded are already in (max_r, max_l)
					for (i32 wi = qn - L - 1; wi >= 0; --wi) {
						const u32 tw = s_q[(qh + wi) & 63][ln];
						rr += s_c[tw][ln]++;
						const i32 new_r = rr, new_l = qn - wi - 1;
						if (new_r * 10 > T * new_l) {
							const i32 thr = wi + start;
							if (occ) {
								for (i32 sv = (folded - 1 < pmax ? folded - 1 : pmax); sv >= thr && sv >= pmin; --sv)
									if (occ >> (sv & 63) & 1) {
										const u32 rl = P[sv & 63].rl;
										const i32 pr = (i32)(rl >> 8), pl = (i32)(rl & 0xff);
										if (max_r == 0 || pr * max_l > max_r * pl) { max_r = pr; max_l = pl; }
									}
								if (thr < folded) folded = thr;
							}
							if (max_r == 0 || new_r * max_l >= max_r * new_l) {
								max_r = new_r; max_l = new_l;
								const u32 idx = (u32)thr & 63u;
								DustPI e; e.finish = qn + 2 + start; e.rl = (u32)new_r << 8 | (u32)new_l;
								if (occ >> idx & 1) {                   // a newer interval of the same start: the bucket keeps its largest r/l
									const u32 rl = P[idx].rl;
									if ((i32)(rl >> 8) * new_l > new_r * (i32)(rl & 0xff)) e.rl = rl;
								} else {
									if (occ == 0) { pmin = thr; pmax = thr; folded = thr; }
									else { if (thr < pmin) pmin = thr; if (thr > pmax) pmax = thr; }
									occ |= 1ULL << idx;
								}
								P[idx] = e;
							}
						}
					}
				}
			}
		}
	}
#undef LQ_DUST_SPLIT_FLUSH
	lq_dust_mask_or(mask, (u32)(s - seq) + (u32)ls, (u32)(s - seq) + (u32)lf);
	}
}

// masked[r] = set bits of mask bits [off[r], off[r + 1]) for every read without a flag; a wave per read
__global__ void __launch_bounds__(LQ_DUST_SPLIT_THREADS)
k_sdust_mask_count(const u32 *mask, const u64 *off, const u8 *flag, u32 n, u32 *masked_out)
{
	const u32 lane = threadIdx.x & 63;
	const u64 wave = (u64)blockIdx.x * (LQ_DUST_SPLIT_THREADS / 64) + threadIdx.x / 64, n_waves = (u64)gridDim.x * (LQ_DUST_SPLIT_THREADS / 64);
	for (u64 r = wave; r < n; r += n_waves) {                      // (wave-uniform)
		if (flag[r]) continue;
		const u64 g0 = off[r], g1 = off[r + 1];
		u32 c = 0;
		if (g1 > g0) {
			const u64 w0 = g0 >> 5, w1 = (g1 - 1) >> 5;
			for (u64 w = w0 + lane; w <= w1; w += 64) {
				u32 m = mask[w];
				if (w == w0) m &= ~0u << (g0 & 31);
				if (w == w1) m &= ~0u >> (31 - ((g1 - 1) & 31));
				c += __popc(m);
			}
		}
		for (int d = 32; d; d >>= 1) c += __shfl_xor(c, d);
		if (lane == 0) masked_out[r] = c;
	}
}

// the quality columns of k_sdust (kernels_dust.hpp:134-147), one thread per read
__global__ void __launch_bounds__(LQ_DUST_THREADS)
k_sdust_qual(const u8 *qual, const u64 *seq_off, u32 n_reads, const double *q2p, double *psum_out, u32 *qv_out)
{
	const u32 tid = blockIdx.x * blockDim.x + threadIdx.x, n_threads = gridDim.x * blockDim.x;
	for (u32 r = tid; r < n_reads; r += n_threads) {
		const u64 off = seq_off[r];
		const i32 len = (i32)(seq_off[r + 1] - off);
		// meanQ's sum (lqutils.c:51-56: sequential, in read order) and getQV(qual, 7) (lqutils.c:61-69); a record without
		// qualities arrives as zero bytes
		double ps = 0.0;
		u32 qv = 0;
		if (qual && len > 0 && qual[off] != 0) {
			const u8 *q = qual + off;
			for (i32 i = 0; i < len; ++i) {
				const i32 v = (i32)(signed char)q[i];                       // (char arithmetic, as lqutils.c:51-56 and k_qual_sum)
				const i32 t = v - 33;
				ps += q2p[t < 0 ? 0 : t > 126 ? 126 : t];                  // the reference indexes out of bounds outside Q0..Q126: clamped, like k_qual_sum
				if (v > 7 + 33) ++qv;
			}
		}
		psum_out[r] = ps; qv_out[r] = qv;
	}
}

// the flagged reads for k_sdust, which walks reads that lie one behind the other: read list[j] of the chunk becomes read j of dst
// (dst_off[0..k]); a block per read, strided
__global__ void __launch_bounds__(LQ_DUST_SPLIT_THREADS)
k_sdust_compact(const u8 *seq, const u64 *seq_off, const u32 *list, const u64 *dst_off, u32 k, u8 *dst)
{
	for (u32 j = blockIdx.x; j < k; j += gridDim.x) {
		const u8 *s = seq + seq_off[list[j]];
		u8 *d = dst + dst_off[j];
		const u64 len = dst_off[j + 1] - dst_off[j];
		for (u64 i = threadIdx.x; i < len; i += LQ_DUST_SPLIT_THREADS) d[i] = s[i];
	}
}

// ... and k_sdust's counts of them back to where the chunk's reads have theirs
__global__ void __launch_bounds__(LQ_DUST_SPLIT_THREADS)
k_sdust_scatter(const u32 *src, const u32 *list, u32 k, u32 *masked_out)
{
	for (u64 j = (u64)blockIdx.x * LQ_DUST_SPLIT_THREADS + threadIdx.x; j < k; j += (u64)gridDim.x * LQ_DUST_SPLIT_THREADS)
		masked_out[list[j]] = src[j];
}
