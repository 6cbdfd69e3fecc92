// longqc_amd/csrc/kernels_chunk.hpp -- the resident chunk's own kernel: the ASCII bases of a chunk of reads, already on the device
// for the per-chunk steps (chunk.cpp), into the engine's packed layout -- what lq_pack_host (engine.cpp) writes on the host and k_pack
// (kernels_sketch.hpp) from a staged upload: every read starts on a 128-base chunk, a chunk is 4 x u64 of 2-bit codes (base j of a
// word at bits 2j..2j+1) and 4 x u32 of "not A/C/G/T/U" bits with the bits beyond the read's end set (seq_nt4_table, sketch.c:8-25:
// either case, U as T, the raw values 0..3 as themselves).  Per read also the flag lq_packed_read_ambiguous computes.
//
// A pure streaming kernel, 1 B per base in and 0.375 B out, no LDS.  One lane makes one packed word (32 bases): four adjacent lanes
// make a chunk, a wave writes 512 contiguous bytes of codes and 256 of bits.  The work list is per block, not per lane: the host
// names the read that holds the first chunk of every tile of 64 chunks (256 words = one block's round), and a lane finds its own
// read by bisecting the at most 65 reads between two such entries -- long and short reads cost a lane the same.  A read begins at
// any byte of the buffer: the lane loads the three aligned 16-byte words that hold its 32 bases (k_gc_reads' scheme: aligned loads,
// the head shifted out, the tail masked) and funnels them down by the start's residue mod 16.  The buffer is allocated 64 bytes past
// the last base, so the third load stays inside for every start.
#pragma once
#include "lq_common.hpp"

#define LQ_PACK_THREADS 256
#define LQ_PACK_TILE_CHUNKS 64u      // chunks of one (block, round): 256 lanes x one word
#define LQ_PACK_MAX_BLOCKS 2048u     // tiles are strided over the blocks of a launch
#define LQ_PACK_PAD 64u              // bytes the sequence buffer extends past the last base

// 0x80 in every byte of x that is zero
__device__ __forceinline__ u32 lq_pk_zero_bytes(u32 x) { return ~(((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x | 0x7f7f7f7fu); }

// four bases (x, first base in the low byte) -> their codes in bits 0..7 (two bits per base, 0 where ambiguous) and, in `bad`,
// bits 0..3 set where a base is none of A/C/G/T/U in either case nor a raw 0..3
__device__ __forceinline__ u32 lq_pk_four(u32 x, u32 &bad)
{
	const u32 f = x & 0xdfdfdfdfu;                                    // upper case
	const u32 acg = lq_pk_zero_bytes((f & 0xf9f9f9f9u) ^ 0x41414141u) & ~lq_pk_zero_bytes(f ^ 0x45454545u);   // 0x41 0x43 0x47, not 0x45
	const u32 tu = lq_pk_zero_bytes((f & 0xfefefefeu) ^ 0x54545454u);                                         // 0x54 0x55
	const u32 raw = lq_pk_zero_bytes(x & 0xfcfcfcfcu);                                                        // 0..3
	const u32 ok = acg | tu | raw;                                    // 0x80 per valid base
	const u32 letter = ((x >> 1) ^ (x >> 2)) & 0x03030303u;           // A 0, C 1, G 2, T and U 3
	const u32 rawm = (raw >> 7) * 3u, okm = (ok >> 7) * 3u;           // 0x03 per byte
	const u32 c = ((letter & ~rawm) | (x & rawm)) & okm;
	const u32 t = (c | (c >> 6)) & 0x000f000fu;
	bad = (((~ok & 0x80808080u) >> 7) * 0x00204081u) >> 21 & 0xfu;
	return (t | (t >> 12)) & 0xffu;
}

__device__ __forceinline__ void lq_pk_eight(u64 q, u64 &w, u32 &m, int at)      // bases 8 * at .. 8 * at + 7 of a word
{
	u32 b0, b1;
	const u32 c0 = lq_pk_four((u32)q, b0), c1 = lq_pk_four((u32)(q >> 32), b1);
	w |= (u64)(c0 | c1 << 8) << (16 * at);
	m |= (b0 | b1 << 4) << (8 * at);
}

// seq: the chunk's bases, read r at soff[r] .. soff[r + 1]; coff[r]: packed chunks before read r; tile_read[t]: the last read r with
// coff[r] <= LQ_PACK_TILE_CHUNKS * t (n_tiles + 1 entries, the last one n_reads - 1).  codes / amb: n_words words.  flags[r] is
// set to 1 when read r holds an ambiguous base (zeroed by the host before the launch; every writer writes the same value).
__global__ void __launch_bounds__(LQ_PACK_THREADS)
k_chunk_pack(const u8 *seq, const u64 *soff, const u64 *coff, const u32 *tile_read, u64 n_tiles, u64 n_words, u64 *codes, u32 *amb, u8 *flags)
{
	for (u64 t = blockIdx.x; t < n_tiles; t += gridDim.x) {
		const u64 g = t * (LQ_PACK_TILE_CHUNKS * LQ_CHUNK_WORDS) + threadIdx.x;
		if (g >= n_words) continue;
		const u64 ch = g / LQ_CHUNK_WORDS;
		u32 lo = tile_read[t], hi = tile_read[t + 1];             // invariant: coff[lo] <= ch, and coff[hi + 1] > ch
		while (lo < hi) {
			const u32 mid = lo + (hi - lo + 1) / 2;
			if (coff[mid] <= ch) lo = mid; else hi = mid - 1;
		}
		const u32 r = lo;
		const u64 s0 = soff[r], len = soff[r + 1] - s0;
		const u64 p0 = (g - coff[r] * LQ_CHUNK_WORDS) * 32;
		const u32 lim = p0 >= len ? 0u : (len - p0 < 32 ? (u32)(len - p0) : 32u);
		u64 w = 0; u32 m = 0;
		if (lim) {
			const u64 a = s0 + p0;
			const uint4 *src = (const uint4*)(seq + (a & ~(u64)15));
			const uint4 v0 = src[0], v1 = src[1], v2 = src[2];
			u64 q0 = (u64)v0.y << 32 | v0.x, q1 = (u64)v0.w << 32 | v0.z, q2 = (u64)v1.y << 32 | v1.x, q3 = (u64)v1.w << 32 | v1.z,
			    q4 = (u64)v2.y << 32 | v2.x;
			const u64 q5 = (u64)v2.w << 32 | v2.z;
			const u32 sh = (u32)(a & 15);
			if (sh & 8) { q0 = q1; q1 = q2; q2 = q3; q3 = q4; q4 = q5; }
			const u32 b = (sh & 7) * 8;
			if (b) { q0 = q0 >> b | q1 << (64 - b); q1 = q1 >> b | q2 << (64 - b); q2 = q2 >> b | q3 << (64 - b); q3 = q3 >> b | q4 << (64 - b); }
			lq_pk_eight(q0, w, m, 0); lq_pk_eight(q1, w, m, 1); lq_pk_eight(q2, w, m, 2); lq_pk_eight(q3, w, m, 3);
			if (lim < 32) { w &= ~0ULL >> (64 - 2 * lim); m &= (1u << lim) - 1u; }      // (what lies behind the read's end is another read's)
			if (m) flags[r] = 1;
		}
		if (lim < 32) m |= lim == 0 ? 0xffffffffu : ~0u << lim;   // beyond the read: ambiguous, as lq_pack_host / k_pack mark it
		codes[g] = w; amb[g] = m;
	}
}
