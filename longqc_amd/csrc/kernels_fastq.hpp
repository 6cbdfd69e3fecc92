// longqc_amd/csrc/kernels_fastq.hpp -- the FASTQ writer's kernel (writer.cpp): the reads of a resident chunk (chunk.hpp), each cut to
// its bases [begin, end), as the text `@name\nseq\n+\nqual\n` -- k_chunk_gather (kernels_gather.hpp) run backwards.  Record i is
//   '@' name '\n' seq[begin:end] '\n' '+' '\n' qual[begin:end] '\n'          name_len + 2 * (end - begin) + 6 bytes
// and the records follow each other without gaps; rec[i] is the text byte at which record i starts (n + 1 entries, the last one the
// text's length), so a name's length is what the record's length leaves: the names travel as lqstore_append takes them (each ends
// with a NUL that the text does not get) and need no table of lengths.
//
// A pure streaming copy, about 2 B in and 2 B out per base, no LDS.  One lane makes one aligned 16-byte word of the text; a block's
// round is a tile of 4096 text bytes.  A launch makes the tiles t0 .. t0 + n_tiles of the text (a piece: the writer streams a chunk's
// text piece by piece, and a piece begins on a tile but at any byte of a record).  The work list is per tile, as k_chunk_gather's: the
// host names the record that holds the first byte of every tile of the text, and a lane finds its own by bisecting rec[] between two
// such entries.  Then the lane walks the fields that fall into its word: mostly one (the middle of a read), up to eleven (three
// records of empty reads with short names).  The bytes of a name, a sequence or a quality string start at any byte of their buffer:
// the lane loads the two aligned 16-byte words that hold the next (at most 16) bytes and funnels them down by the start's residue
// mod 16, as the gather does; all three buffers extend LQ_GATHER_SRC_PAD bytes past their last byte, so the second load stays inside.
// Bytes of the last word behind the text's end are written as zero.
#pragma once
#include "chunk.hpp"

#define LQ_FASTQ_THREADS 256
#define LQ_FASTQ_TILE 4096u          // text bytes of one (block, round): 256 lanes x 16 bytes
#define LQ_FASTQ_MAX_BLOCKS 2048u    // tiles are strided over the blocks of a launch

// be[i]: (begin, end) of read i, in bases of the read.  tile_rec[t]: the last record r with rec[r] <= LQ_FASTQ_TILE * t, for every tile
// of the whole text and one more entry (n - 1).  dst: the launch's first byte (text byte LQ_FASTQ_TILE * t0), whole 16-byte words.
__global__ void __launch_bounds__(LQ_FASTQ_THREADS)
k_fastq_format(const u8 *seq, const u8 *qual, const u64 *off, const u8 *names, const u64 *name_off, const uint2 *be, const u64 *rec,
               const u32 *tile_rec, u64 t0, u64 n_tiles, u64 total, u8 *dst)
{
	for (u64 t = blockIdx.x; t < n_tiles; t += gridDim.x) {
		const u64 d0 = (t0 + t) * LQ_FASTQ_TILE + (u64)threadIdx.x * 16;
		if (d0 >= total) continue;
		u32 lo = tile_rec[t0 + t], hi = tile_rec[t0 + t + 1];         // invariant: rec[lo] <= d0, and rec[hi + 1] > d0
		while (lo < hi) {
			const u32 mid = lo + (hi - lo + 1) / 2;
			if (rec[mid] <= d0) lo = mid; else hi = mid - 1;
		}
		u32 r = lo;
		u64 wl = 0, wh = 0;                                       // the word: bytes 0..7, 8..15
		const u32 want = total - d0 < 16 ? (u32)(total - d0) : 16u;
		u64 rs = rec[r], rn = rec[r + 1];
		uint2 b = be[r];
		for (u32 f = 0; f < want;) {                              // f: bytes of the word made so far
			// the record's fields end at: '@' 1, name e1, '\n' e1 + 1, bases e2, "\n+\n" e2 + 3, qualities e3, '\n' e3 + 1
			const u64 m = b.y - b.x, e1 = rn - rs - 5 - 2 * m, e2 = e1 + 1 + m, e3 = e2 + 3 + m;
			const u64 p = d0 + f - rs;                            // the next byte's place in the record
			const u8 *src = nullptr;
			u64 q0 = '\n', q1 = 0, k = 1;                            // the field's next bytes (up to 16), and how many it still has
			if (p == 0) q0 = '@';
			else if (p < e1) { src = names + name_off[r] + (p - 1); k = e1 - p; }
			else if (p == e1) ;
			else if (p < e2) { src = seq + off[r] + b.x + (p - e1 - 1); k = e2 - p; }
			else if (p < e2 + 3) { q0 = 0x0a2b0aULL >> 8 * (u32)(p - e2); k = e2 + 3 - p; }
			else if (p < e3) { src = qual + off[r] + b.x + (p - e2 - 3); k = e3 - p; }
			const u32 c = k < want - f ? (u32)k : want - f;       // bytes this field gives: 1..16
			if (src) {
				const uint4 *s16 = (const uint4*)((uintptr_t)src & ~(uintptr_t)15);
				const uint4 v0 = s16[0], v1 = s16[1];
				q0 = (u64)v0.y << 32 | v0.x; q1 = (u64)v0.w << 32 | v0.z;
				u64 q2 = (u64)v1.y << 32 | v1.x;
				const u64 q3 = (u64)v1.w << 32 | v1.z;
				const u32 sh = (u32)((uintptr_t)src & 15);
				if (sh & 8) { q0 = q1; q1 = q2; q2 = q3; }
				const u32 bits = (sh & 7) * 8;
				if (bits) { q0 = q0 >> bits | q1 << (64 - bits); q1 = q1 >> bits | q2 << (64 - bits); }
			}
			if (c < 8) { q0 &= ~0ULL >> (64 - 8 * c); q1 = 0; }
			else if (c < 16) q1 = c == 8 ? 0 : q1 & ~0ULL >> (128 - 8 * c);
			if (f >= 8) wh |= q0 << (8 * (f - 8));
			else if (f) { wl |= q0 << (8 * f); wh |= q0 >> (64 - 8 * f) | q1 << (8 * f); }
			else { wl = q0; wh = q1; }
			f += c;
			if (f < want && d0 + f == rn) { rs = rn; rn = rec[++r + 1]; b = be[r]; }
		}
		uint4 o;
		o.x = (u32)wl; o.y = (u32)(wl >> 32); o.z = (u32)wh; o.w = (u32)(wh >> 32);
		*(uint4*)(dst + t * LQ_FASTQ_TILE + (u64)threadIdx.x * 16) = o;
	}
}
