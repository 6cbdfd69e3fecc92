// longqc_amd/csrc/kernels_gather.hpp -- the file reader's kernel (reader.cpp): the raw bytes of a FASTA/FASTQ file, uploaded as they
// were read, into the flat sequence and quality buffers of a resident chunk (chunk.hpp) -- the layout lqchunk_load leaves.  The host
// has parsed the bytes into segments: a segment is a run of source bytes (one line of a sequence or of a quality string, without its
// line break and without the '\r' kseq drops) that lands at one place of the destination; the segments of a buffer follow each other
// in the destination without gaps, so a segment's length is the distance to the next one's destination.  A record without a quality
// string has one segment without a source (LQ_GATHER_FILL): '!' for every base, as lq_utils.parse_fastx_chunk gives it.
//
// A pure streaming copy, 1 B in and 1 B out per byte, no LDS.  One lane makes one aligned 16-byte word of the destination; a block's
// round is a tile of 4096 destination bytes.  The work list is per tile, as k_chunk_pack's tile_read: the host names the segment that
// holds the first byte of every tile, and a lane finds its own by bisecting the segments between two such entries -- long and short
// lines cost a lane the same.  A destination word spans one segment (a read on one line), two (a FASTA wrapped at 60 columns) or up
// to 16 (one column): the lane walks them.  A segment starts at any byte of the source: the lane loads the two aligned 16-byte words
// that hold its next (at most 16) bytes and funnels them down by the start's residue mod 16 (k_gc_reads' and k_chunk_pack's scheme);
// the source buffer is allocated LQ_GATHER_SRC_PAD bytes past its last byte, so the second load stays inside for every start.
// Bytes of the last word behind the last destination byte are written as zero.
#pragma once
#include "chunk.hpp"

#define LQ_GATHER_THREADS 256
#define LQ_GATHER_TILE 4096u         // destination bytes of one (block, round): 256 lanes x 16 bytes
#define LQ_GATHER_MAX_BLOCKS 2048u   // tiles are strided over the blocks of a launch
// (GatherSeg, LQ_GATHER_FILL and LQ_GATHER_SRC_PAD: chunk.hpp, where the reader sees them)

// a..z -> A..Z in every byte of x, every other byte (those of 0x80 and more included) as it is
__device__ __forceinline__ u64 lq_ga_upper(u64 x)
{
	const u64 l7 = x & 0x7f7f7f7f7f7f7f7fULL;
	const u64 ge_a = l7 + 0x1f1f1f1f1f1f1f1fULL, gt_z = l7 + 0x0505050505050505ULL;      // bit 7: the low seven bits are >= 'a' / > 'z'
	return x ^ ((ge_a & ~gt_z & ~x & 0x8080808080808080ULL) >> 2);
}

// segs: n_segs segments and one more entry whose dst is `total`; tile_seg[t]: the last segment s with segs[s].dst <= LQ_GATHER_TILE * t
// (n_tiles + 1 entries, the last one n_segs - 1).  dst: whole 16-byte words up to `total` rounded up.
__global__ void __launch_bounds__(LQ_GATHER_THREADS)
k_chunk_gather(const u8 *raw, const GatherSeg *segs, const u32 *tile_seg, u64 n_tiles, u64 total, u8 *dst, int upper)
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
			const u32 m = next - d < want - f ? (u32)(next - d) : want - f;      // bytes this segment gives: 1..16
			u64 q0, q1;
			if (sg.src == LQ_GATHER_FILL) q0 = q1 = 0x2121212121212121ULL;
			else {
				const u64 a = sg.src + (d - sg.dst);
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
			if (m < 8) { q0 &= ~0ULL >> (64 - 8 * m); q1 = 0; }      // (what lies behind the segment's end is a line break, or another line)
			else if (m < 16) q1 = m == 8 ? 0 : q1 & ~0ULL >> (128 - 8 * m);
			if (f >= 8) wh |= q0 << (8 * (f - 8));
			else if (f) { wl |= q0 << (8 * f); wh |= q0 >> (64 - 8 * f) | q1 << (8 * f); }
			else { wl = q0; wh = q1; }
			f += m;
			if (f < want) sg = segs[++s];
		}
		if (upper) { wl = lq_ga_upper(wl); wh = lq_ga_upper(wh); }
		uint4 o;
		o.x = (u32)wl; o.y = (u32)(wl >> 32); o.z = (u32)wh; o.w = (u32)(wh >> 32);
		*(uint4*)(dst + d0) = o;
	}
}
