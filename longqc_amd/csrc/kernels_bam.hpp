// longqc_amd/csrc/kernels_bam.hpp -- the file reader's kernels for BAM (reader.cpp): the inflated bytes of an unaligned BAM file,
// uploaded as they were inflated, into the flat sequence and quality buffers of a resident chunk -- what lq_utils.parse_bam_chunk
// (lq_utils.py:238-261) makes of pysam's records, without the bases ever being text on the host.  The destination layout, the tile,
// the launch cap and the per-tile segment table with bisection are k_chunk_gather's (kernels_gather.hpp).
//
// k_bam_gather: a segment is one read's packed sequence -- src: the byte of its first two bases, dst: its first base in the flat
// buffer.  BAM packs two bases per byte, the first in the high nibble, in the code table "=ACMGRSVTWYHKDBN"; a read always starts on
// a high nibble, but reads lie back to back in the destination, so the 16 bases of a lane start at base k = d - seg.dst of either
// parity and may span many reads (reads without bases have no segment).  For every segment that gives bases the lane loads the two
// aligned 16-byte words that hold the (at most 9) bytes it needs, funnels them down by the start's residue mod 16 and, for an odd k,
// by four more bits; the 8 bytes are spread to 16 codes and looked up in the table, which is four registers: two byte permutes on
// the low three bits of a code and a select on the fourth.  0.5 B in and 1 B out per base, no LDS, no memory table.
//
// k_bam_qual (is_sequel=False, lq_utils.py:253): a segment is one read's quality bytes, which become chr(q + 33): the byte gather of
// k_chunk_gather with 33 added modulo 256.  A read whose first quality byte is 0xff has no qualities (SAM 4.2.3) and gets '!', as a
// segment without a source does.  With is_sequel=True (the default) the qualities are '!' throughout and k_chunk_gather's
// LQ_GATHER_FILL segments make them; no BAM kernel runs for them.
#pragma once
#include "kernels_gather.hpp"

// v_perm_b32 for selectors 0..7: byte i of the result is byte sel.byte[i] of hi:lo
__device__ __forceinline__ u32 lq_bam_perm(u32 hi, u32 lo, u32 sel)
{
#ifdef LQ_EMU
	const u64 v = (u64)hi << 32 | lo;
	u32 r = 0;
	for (int i = 0; i < 4; ++i) r |= (u32)((v >> (8 * ((sel >> (8 * i)) & 7))) & 0xff) << (8 * i);
	return r;
#else
	return __builtin_amdgcn_perm(hi, lo, sel);
#endif
}

// four codes 0..15, one per byte -> their letters in "=ACMGRSVTWYHKDBN"
__device__ __forceinline__ u32 lq_bam_letters(u32 c)
{
	const u32 sel = c & 0x07070707u;
	const u32 a = lq_bam_perm(0x56535247u, 0x4d43413du, sel);      // "GRSV" : "=ACM"
	const u32 b = lq_bam_perm(0x4e42444bu, 0x48595754u, sel);      // "KDBN" : "TWYH"
	const u32 m = ((c >> 3) & 0x01010101u) * 0xffu;
	return a ^ ((a ^ b) & m);
}

// four packed bytes (eight bases, the first in the high nibble of the lowest byte) -> eight letters
__device__ __forceinline__ u64 lq_bam_expand(u32 p)
{
	u64 x = p;
	x = (x | x << 16) & 0x0000ffff0000ffffULL;
	x = (x | x << 8) & 0x00ff00ff00ff00ffULL;                    // byte 2i: packed byte i
	x = (x >> 4 & 0x000f000f000f000fULL) | (x & 0x000f000f000f000fULL) << 8;
	return (u64)lq_bam_letters((u32)(x >> 32)) << 32 | lq_bam_letters((u32)x);
}

// bytes a .. a + 15 of raw in q0 (a .. a + 7) and q1: two aligned loads, funnelled down (k_chunk_gather's scheme)
__device__ __forceinline__ void lq_bam_load16(const u8 *raw, u64 a, u64 &q0, u64 &q1)
{
	const uint4 *src = (const uint4*)(raw + (a & ~(u64)15));
	const uint4 v0 = src[0], v1 = src[1];
	q0 = (u64)v0.y << 32 | v0.x; q1 = (u64)v0.w << 32 | v0.z;
	u64 q2 = (u64)v1.y << 32 | v1.x;
	const u64 q3 = (u64)v1.w << 32 | v1.z;
	const u32 sh = (u32)(a & 15);
	if (sh & 8) { q0 = q1; q1 = q2; q2 = q3; }
	const u32 b = (sh & 7) * 8;
	if (b) { q0 = q0 >> b | q1 << (64 - b); q1 = q1 >> b | q2 << (64 - b); }
}

// QUAL false: the sequences; true: the qualities.  Arguments as k_chunk_gather's.
template <bool QUAL>
__device__ __forceinline__ void lq_bam_gather(const u8 *raw, const GatherSeg *segs, const u32 *tile_seg, u64 n_tiles, u64 total, u8 *dst)
{
	for (u64 t = blockIdx.x; t < n_tiles; t += gridDim.x) {
		const u64 d0 = t * LQ_GATHER_TILE + (u64)threadIdx.x * 16;
		if (d0 >= total) continue;
		u32 lo = tile_seg[t], hi = tile_seg[t + 1];               // invariant: segs[lo].dst <= d0, and segs[hi + 1].dst > d0
		while (lo < hi) {
			const u32 mid = lo + (hi - lo + 1) / 2;
			if (segs[mid].dst <= d0) lo = mid; else hi = mid - 1;
		}
		u32 s = lo;
		u64 wl = 0, wh = 0;                                       // the word: bytes 0..7, 8..15
		const u32 want = total - d0 < 16 ? (u32)(total - d0) : 16u;
		GatherSeg sg = segs[s];
		for (u32 f = 0; f < want;) {                              // f: bytes of the word made so far
			const u64 next = segs[s + 1].dst, d = d0 + f;
			const u32 m = next - d < want - f ? (u32)(next - d) : want - f;      // bases this read gives: 1..16
			const u64 k = d - sg.dst;                                 // the first of them in its read
			u64 q0, q1;
			if (QUAL) {
				if (sg.src == LQ_GATHER_FILL || raw[sg.src] == 0xff) q0 = q1 = 0x2121212121212121ULL;
				else {
					lq_bam_load16(raw, sg.src + k, q0, q1);
					q0 = ((q0 & 0x7f7f7f7f7f7f7f7fULL) + 0x2121212121212121ULL) ^ (q0 & 0x8080808080808080ULL);      // + 33 in every byte
					q1 = ((q1 & 0x7f7f7f7f7f7f7f7fULL) + 0x2121212121212121ULL) ^ (q1 & 0x8080808080808080ULL);
				}
			} else {
				u64 p, p1;
				lq_bam_load16(raw, sg.src + (k >> 1), p, p1);
				if (k & 1)                                            // byte i: the low nibble of byte i and the high nibble of byte i + 1
					p = (p & 0x0f0f0f0f0f0f0f0fULL) << 4 | (p >> 12 & 0x000f0f0f0f0f0f0fULL) | (p1 >> 4 & 15) << 56;
				q0 = lq_bam_expand((u32)p); q1 = lq_bam_expand((u32)(p >> 32));
			}
			if (m < 8) { q0 &= ~0ULL >> (64 - 8 * m); q1 = 0; }      // (what lies behind the read's end is its qualities, or another record)
			else if (m < 16) q1 = m == 8 ? 0 : q1 & ~0ULL >> (128 - 8 * m);
			if (f >= 8) wh |= q0 << (8 * (f - 8));
			else if (f) { wl |= q0 << (8 * f); wh |= q0 >> (64 - 8 * f) | q1 << (8 * f); }
			else { wl = q0; wh = q1; }
			f += m;
			if (f < want) sg = segs[++s];
		}
		uint4 o;
		o.x = (u32)wl; o.y = (u32)(wl >> 32); o.z = (u32)wh; o.w = (u32)(wh >> 32);
		*(uint4*)(dst + d0) = o;
	}
}

// segs, tile_seg, n_tiles, total, dst: as k_chunk_gather's; raw: the inflated bytes, LQ_GATHER_SRC_PAD bytes allocated past the last
__global__ void __launch_bounds__(LQ_GATHER_THREADS)
k_bam_gather(const u8 *raw, const GatherSeg *segs, const u32 *tile_seg, u64 n_tiles, u64 total, u8 *dst)
{
	lq_bam_gather<false>(raw, segs, tile_seg, n_tiles, total, dst);
}

__global__ void __launch_bounds__(LQ_GATHER_THREADS)
k_bam_qual(const u8 *raw, const GatherSeg *segs, const u32 *tile_seg, u64 n_tiles, u64 total, u8 *dst)
{
	lq_bam_gather<true>(raw, segs, tile_seg, n_tiles, total, dst);
}
