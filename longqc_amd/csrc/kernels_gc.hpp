// longqc_amd/csrc/kernels_gc.hpp -- the GC fraction step of LongQC's sampleqc (lq_gcfrac.py:25-48): per read the number of
// 'G' and 'C' bytes, per sampled position i the number of them in seq[i : min(i + cs, l)], and per read the index (in draw
// order) of the first position the reference's walk stops at (i + cs - 1 > l).  Every result is an integer; the divisions
// and the float32 roundings are the host's (longqc_amd/gcfrac.py), so they are the reference's own IEEE operations.
//
// The host hands the kernels one span [b0, b1) of the chunk's concatenated ASCII sequence at a time (b0 a multiple of
// LQ_GC_TILE; buf points at byte b0 of the resident chunk, chunk.hpp, which holds whole tiles), so that a window which starts
// inside the span can be read to its end behind b1.  A read may lie in several spans: gc[] and kept[] live on the device for the whole call and are updated with
// integer atomics, which makes the result independent of the spans and of the order of the waves.
//   k_gc_reads    a wave takes one aligned tile of LQ_GC_TILE bytes of the span (4 x 16-byte loads per lane) and then visits
//                 the reads that overlap the tile, one (read, tile) item after the other: bytes outside the read are masked
//                 out of the per-word counts, the wave reduces, lane 0 adds once.  A tile inside one long read is one item
//                 without masks; a tile over many short reads is one item per read on data already in registers.
//   k_gc_draw     position j of read g = the image of j under a keyed bijection of [0, l) (below): the device's draw.
//   k_gc_windows  16 lanes per drawn position: 16-byte loads over the window's aligned words, masked to [a, e), a shuffle
//                 reduction of width 16.  The span a window starts in owns it (count and the kept[] minimum).
#pragma once
#include "lq_common.hpp"

#define LQ_GC_THREADS 256
#define LQ_GC_TILE 4096u             // bytes of one (wave, tile): 64 lanes x 4 loads x 16 bytes
#define LQ_GC_MAXCS 4096u            // largest chunk_size: a window count fits 16 bits, and the upload margin covers a window
#define LQ_GC_MAX_BLOCKS 2048u       // tiles / windows / draws are strided over the blocks of a launch
#define LQ_GC_ROUNDS 6               // Feistel rounds of the draw

// ---- the device draw --------------------------------------------------------------------------------------------------
// lq_gc_mix64 is splitmix64's output function of z + 0x9e3779b97f4a7c15, lq_gc_mix32 is MurmurHash3's 32-bit finalizer.
// Keys of read g (its ordinal in the whole input) under `seed`: a = mix64(mix64(seed) ^ g), b = mix64(a), c = mix64(b);
// round keys rk[0..5] = lo32(a), hi32(a), lo32(b), hi32(b), lo32(c), hi32(c).  h = the smallest h >= 1 with 4^h >= l.
// E(x), x < 4^h: (L, R) = (x >> h, x & (2^h - 1)); six times (L, R) = (R, L ^ (mix32(R ^ rk[r]) & (2^h - 1))); L << h | R.
// E is a bijection of [0, 4^h) (a balanced Feistel network); position j = E applied to j until the value is below l (cycle
// walking), which is a bijection of [0, l): the k positions j = 0..k-1 are distinct.  4^h < 4 l, so a walk takes under four
// applications on average.
__host__ __device__ __forceinline__ u64 lq_gc_mix64(u64 z)
{
	z += 0x9e3779b97f4a7c15ULL;
	z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ULL;
	z = (z ^ (z >> 27)) * 0x94d049bb133111ebULL;
	return z ^ (z >> 31);
}

__host__ __device__ __forceinline__ u32 lq_gc_mix32(u32 x)
{
	x ^= x >> 16; x *= 0x85ebca6bu;
	x ^= x >> 13; x *= 0xc2b2ae35u;
	return x ^ (x >> 16);
}

__host__ __device__ __forceinline__ u32 lq_gc_draw_pos(u64 seed, u64 g, u32 l, u32 j)
{
	u32 rk[LQ_GC_ROUNDS];
	u64 a = lq_gc_mix64(lq_gc_mix64(seed) ^ g);
	for (int r = 0; r < LQ_GC_ROUNDS; r += 2) { rk[r] = (u32)a; rk[r + 1] = (u32)(a >> 32); a = lq_gc_mix64(a); }
	u32 h = 1;
	while (h < 16 && (1ULL << (2 * h)) < (u64)l) ++h;
	const u32 m = (1u << h) - 1;
	u32 x = j;
	do {
		u32 L = x >> h, R = x & m;
		for (int r = 0; r < LQ_GC_ROUNDS; ++r) { const u32 t = L ^ (lq_gc_mix32(R ^ rk[r]) & m); L = R; R = t; }
		x = L << h | R;
	} while (x >= l);
	return x;
}

// ---- helpers ----------------------------------------------------------------------------------------------------------
// the last r in [0, n] with off[r] <= x (off ascending, off[0] <= x): the read -- or the draw's read -- that holds x, empty ones skipped
__device__ __forceinline__ u32 lq_gc_find(const u64 *off, u32 n, u64 x)
{
	u32 lo = 0, hi = n;                                       // invariant: off[lo] <= x, and off[hi + 1] > x or hi == n
	while (lo < hi) {
		const u32 mid = lo + (hi - lo + 1) / 2;
		if (off[mid] <= x) lo = mid; else hi = mid - 1;
	}
	return lo;
}

// 0x80 in every byte of x that is 'C' (0x43) or 'G' (0x47): the two differ in bit 2 alone
__device__ __forceinline__ u32 lq_gc_hits(u32 x)
{
	const u32 y = (x & 0xfbfbfbfbu) ^ 0x43434343u;            // a zero byte where x had C or G
	return ~(((y & 0x7f7f7f7fu) + 0x7f7f7f7fu) | y | 0x7f7f7f7fu);
}

// 0x80 in every byte of the word at offset a whose offset lies in [lo, hi) (offsets inside a tile or a window: 32 bits do)
__device__ __forceinline__ u32 lq_gc_mask(u32 a, u32 lo, u32 hi)
{
	const u32 s = lo > a ? (lo - a < 4 ? lo - a : 4u) : 0u;   // bytes before lo
	const u32 e = hi > a ? (hi - a < 4 ? hi - a : 4u) : 0u;   // bytes before hi
	const u32 ml = s >= 4 ? 0u : 0x80808080u << (8 * s);
	const u32 mh = e >= 4 ? 0x80808080u : 0x80808080u & ((1u << (8 * e)) - 1u);
	return ml & mh;
}

__device__ __forceinline__ u32 lq_gc_count16(const uint4 &v) { return __popc(lq_gc_hits(v.x)) + __popc(lq_gc_hits(v.y)) + __popc(lq_gc_hits(v.z)) + __popc(lq_gc_hits(v.w)); }

__device__ __forceinline__ u32 lq_gc_count16_masked(const uint4 &v, u32 a, u32 lo, u32 hi)
{
	return __popc(lq_gc_hits(v.x) & lq_gc_mask(a, lo, hi)) + __popc(lq_gc_hits(v.y) & lq_gc_mask(a + 4, lo, hi))
	     + __popc(lq_gc_hits(v.z) & lq_gc_mask(a + 8, lo, hi)) + __popc(lq_gc_hits(v.w) & lq_gc_mask(a + 12, lo, hi));
}

// ---- kernels ----------------------------------------------------------------------------------------------------------
// buf holds the sequence from byte b0 on, allocated up to a multiple of LQ_GC_TILE; off[0..n] are the reads' offsets
// in the whole sequence.  gc[r] += G/C bytes of read r inside [b0, b1).
__global__ void __launch_bounds__(LQ_GC_THREADS)
k_gc_reads(const u8 *buf, u64 b0, u64 b1, const u64 *off, u32 n, u32 *gc)
{
	const u32 lane = threadIdx.x & 63;
	const u64 n_tiles = (b1 - b0 + LQ_GC_TILE - 1) / LQ_GC_TILE;
	const u64 wave = (u64)blockIdx.x * (LQ_GC_THREADS / 64) + threadIdx.x / 64, n_waves = (u64)gridDim.x * (LQ_GC_THREADS / 64);
	for (u64 t = wave; t < n_tiles; t += n_waves) {
		const u64 A = b0 + t * LQ_GC_TILE, Aend = A + LQ_GC_TILE < b1 ? A + LQ_GC_TILE : b1;
		const uint4 *src = (const uint4*)(buf + (A - b0));
		uint4 v[4];
		for (int i = 0; i < 4; ++i) v[i] = src[i * 64 + lane];
		for (u32 r = lq_gc_find(off, n, A); r < n; ++r) {      // (wave-uniform: every lane walks the same reads)
			const u64 lo = off[r], hi = off[r + 1];
			if (lo >= Aend) break;
			if (hi == lo) continue;
			u32 c = 0;
			if (lo <= A && hi >= A + LQ_GC_TILE) {
				for (int i = 0; i < 4; ++i) c += lq_gc_count16(v[i]);
			} else {
				const u32 m_lo = lo > A ? (u32)(lo - A) : 0u, m_hi = (u32)((hi < Aend ? hi : Aend) - A);       // offsets in the tile
				for (int i = 0; i < 4; ++i) c += lq_gc_count16_masked(v[i], (u32)(i * 64 + lane) * 16, m_lo, m_hi);
			}
			for (int d = 32; d; d >>= 1) c += __shfl_xor(c, d);
			if (lane == 0 && c) atomicAdd(gc + r, c);
		}
	}
}

// pos[d] for the draws d of draw_off[0..n]: draw j = d - draw_off[r] of read r, whose ordinal in the input is first_read + r
__global__ void __launch_bounds__(LQ_GC_THREADS)
k_gc_draw(const u64 *off, const u64 *draw_off, u32 n, u64 seed, u64 first_read, u32 *pos)
{
	const u64 n_draws = draw_off[n];
	for (u64 d = (u64)blockIdx.x * LQ_GC_THREADS + threadIdx.x; d < n_draws; d += (u64)gridDim.x * LQ_GC_THREADS) {
		const u32 r = lq_gc_find(draw_off, n, d);
		pos[d] = lq_gc_draw_pos(seed, first_read + r, (u32)(off[r + 1] - off[r]), (u32)(d - draw_off[r]));
	}
}

// draws [d_lo, d_hi) (those of the reads that overlap [b0, b1)); a draw whose window starts at a byte of [b0, b1) is this
// launch's: win[d] = G/C bytes of the window cut at the read's end, kept[r] = min(kept[r], j) if the walk stops at draw j
__global__ void __launch_bounds__(LQ_GC_THREADS)
k_gc_windows(const u8 *buf, u64 b0, u64 b1, const u64 *off, const u64 *draw_off, u32 n, const u32 *pos, u32 cs,
             u64 d_lo, u64 d_hi, u16 *win, u32 *kept)
{
	const u32 sub = threadIdx.x & 15;
	const u64 grp = ((u64)blockIdx.x * LQ_GC_THREADS + threadIdx.x) / 16, n_grp = (u64)gridDim.x * (LQ_GC_THREADS / 16);
	const u64 n_iter = (d_hi - d_lo + n_grp - 1) / n_grp;      // (the same for every lane: the shuffles below run converged)
	for (u64 it = 0; it < n_iter; ++it) {
		const u64 d = d_lo + it * n_grp + grp;
		u32 c = 0, r = 0;
		bool own = false;
		if (d < d_hi) {
			r = lq_gc_find(draw_off, n, d);
			const u64 lo = off[r], hi = off[r + 1];
			const u32 i = pos[d];
			const u64 a = lo + i;
			own = a >= b0 && a < b1;
			if (own) {
				if (sub == 0 && (u64)i + cs - 1 > hi - lo) atomicMin(kept + r, (u32)(d - draw_off[r]));
				const u64 e = a + cs < hi ? a + cs : hi;
				const u64 base = a & ~(u64)15;                       // (>= b0: b0 is a multiple of the tile)
				const u32 a_rel = (u32)(a - base), e_rel = (u32)(e - base);
				for (u32 w = 16 * sub; w < e_rel; w += 256)
					c += lq_gc_count16_masked(*(const uint4*)(buf + (base - b0) + w), w, a_rel, e_rel);
			}
		}
		for (int s = 8; s; s >>= 1) c += __shfl_xor(c, s, 16);
		if (own && sub == 0) win[d] = (u16)c;
	}
}
