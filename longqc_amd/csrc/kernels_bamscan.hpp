// longqc_amd/csrc/kernels_bamscan.hpp -- the record walk of an unaligned BAM on the device (reader.cpp, lqreader_bam_walk): the
// records of a range of inflated BAM bytes that lie on the device, found there, as rows (FxRow, FxInfo) and the GatherSeg lists
// k_bam_gather / k_bam_qual (kernels_bam.hpp) take -- the shape of the FASTA/FASTQ scan's result (kernels_fxscan.hpp).  The record
// layout is the SAM/BAM specification's 4.2 as reader.cpp::parse_bam_one reads it; the scan answers only for records it can vouch for
// (DESIGN 8 (15) has the domain) and names the position from which parse_bam_one goes on.
//
// A BAM record says where the next one starts, so the records are a linked chain from the range's start.  No lane follows it:
//   k_bam_candidates a streaming pass over the bytes, 16 offsets per lane: the offsets that pass the cheap part of the test -- bytes
//                    o+4 .. o+11 and o+24 .. o+31 all 0xff (refID, pos, next_refID, next_pos of an unaligned record), l_seq's top bit
//                    clear, 36 bytes inside the range -- counted per tile (phase 0) and, after k_fx_tilescan, listed ascending
//                    (phase 1).  Entry 0 is the range's start whatever its bytes say.
//   k_bam_link       one lane per candidate: the full test, and the index of next(o) = o + 4 + block_size among the candidates by
//                    bisection: link[i] and jump[i].
//   k_fx_jump        (kernels_fxscan.hpp, as it is) marks the candidates reachable from entry 0, one launch per doubling.  A false
//                    candidate -- tag bytes that look like a record, a run of 0xff qualities -- is harmless only because nothing but
//                    entry 0 starts marked.
//   k_bam_emit       counts rows, segments and bases of the marked, vouched candidates per tile (phase 0) and, after k_fx_tilescan,
//                    writes rows, infos, one sequence and one quality segment per record with bases, and the resume word (phase 1).
// Tiles, threads and the block cap are LQ_FXSCAN_*'s; positions are 32-bit.  LDS: one word per wave for the block scans.
#pragma once
#include "kernels_fxscan.hpp"

#define LQ_BAMSCAN_EMIT_COLS 3        // k_bam_emit's counts per tile: records, segments (of either list), bases
static_assert(LQ_FXSCAN_LINE_TILE <= 0x3ffu, "k_bam_emit packs a tile's record and segment counts into 10 bits each");

// bits 0..3: bytes 0..3 of x are 0xff
__device__ __forceinline__ u32 lq_bam_ff4(u32 x)
{
	const u32 t = x & 0x80808080u & ((x & 0x7f7f7f7fu) + 0x01010101u);
	return (t >> 7 & 1) | (t >> 14 & 2) | (t >> 21 & 4) | (t >> 28 & 8);
}
// bit k: byte k of the 16 is 0xff
__device__ __forceinline__ u64 lq_bam_ff16(const uint4 v)
{
	return (u64)(lq_bam_ff4(v.x) | lq_bam_ff4(v.y) << 4 | lq_bam_ff4(v.z) << 8 | lq_bam_ff4(v.w) << 12);
}
__device__ __forceinline__ u32 lq_bam_le32(const u8 *p) { return (u32)p[0] | (u32)p[1] << 8 | (u32)p[2] << 16 | (u32)p[3] << 24; }

// base: the bytes, 16-byte aligned, base + hi + 16 readable; the range is base[lo .. hi), lo a record boundary.  Tile t is
// base[(lo & ~15) + 4096 t ..).  phase 0: cols[t] = the tile's candidates (the offsets above lo that pass the cheap test).  phase 1
// (cols scanned): cand[0] = lo, cand[1 + k] = the k-th of them.
static __global__ void __launch_bounds__(LQ_FXSCAN_THREADS, 8)       // (eight waves per SIMD: a streaming pass)
k_bam_candidates(const u8 *base, u32 lo, u32 hi, u64 n_tiles, u64 *cols, int phase, u32 *cand)
{
	__shared__ u64 wsum[LQ_FXSCAN_THREADS / 64];
	const u32 t0 = lo & ~15u;
	if (phase && blockIdx.x == 0 && threadIdx.x == 0) cand[0] = lo;
	for (u64 t = blockIdx.x; t < n_tiles; t += gridDim.x) {
		const u64 w64 = (u64)t0 + t * LQ_FXSCAN_TILE + (u64)threadIdx.x * 16;
		u32 hits = 0;                                             // bit k: offset w64 + k is a candidate
		if (w64 + 36 <= hi) {                                     // (a word is loaded only if its first byte lies inside the range)
			const u8 *p = base + w64;
			uint4 z; z.x = z.y = z.z = z.w = 0;
			const uint4 v0 = *(const uint4*)p, v1 = *(const uint4*)(p + 16), v2 = w64 + 32 < hi ? *(const uint4*)(p + 32) : z;
			const u64 ff = lq_bam_ff16(v0) | lq_bam_ff16(v1) << 16 | lq_bam_ff16(v2) << 32;      // bit k: byte w64 + k is 0xff
			// the top bits of bytes 16 .. 47: byte k + 23 is the high byte of l_seq
			const u64 top = (u64)(lq_bam_ff4(v1.x | 0x7f7f7f7fu) | lq_bam_ff4(v1.y | 0x7f7f7f7fu) << 4 | lq_bam_ff4(v1.z | 0x7f7f7f7fu) << 8 | lq_bam_ff4(v1.w | 0x7f7f7f7fu) << 12) << 16
			              | (u64)(lq_bam_ff4(v2.x | 0x7f7f7f7fu) | lq_bam_ff4(v2.y | 0x7f7f7f7fu) << 4 | lq_bam_ff4(v2.z | 0x7f7f7f7fu) << 8 | lq_bam_ff4(v2.w | 0x7f7f7f7fu) << 12) << 32;
			if (ff) {
				#pragma unroll
				for (u32 k = 0; k < 16; ++k) {
					const bool ok = (ff >> (k + 4) & 0xff) == 0xff && (ff >> (k + 24) & 0xff) == 0xff && !(top >> (k + 23) & 1);
					if (ok && w64 + k > lo && w64 + k + 36 <= hi) hits |= 1u << k;
				}
			}
		}
		u64 tot;
		const u64 ex = lq_fx_block_scan((u64)__popc(hits), wsum, &tot);
		if (!phase) { if (threadIdx.x == 0) cols[t] = tot; continue; }
		u64 at = 1 + cols[t] + ex;
		for (u32 h = hits; h; h &= h - 1) cand[at++] = (u32)w64 + (u32)(__ffs(h) - 1);
	}
}

// link[i] = {next(o), l_seq | vouched << 31, the first byte of the packed sequence, jump[i]} for o = cand[i]; a candidate that fails
// the full test has bit 31 of .y clear.  jump[i] = the index of next(o) among the candidates, or n_cand if the test fails or next(o) is
// none (k_fx_jump doubles the jumps in place: link keeps the first); jump[n_cand] = n_cand.  mark[i] = 1 for entry 0, else 0.
static __global__ void __launch_bounds__(LQ_FXSCAN_THREADS)
k_bam_link(const u8 *base, u32 hi, const u32 *cand, u32 n_cand, uint4 *link, u32 *jump, u32 *mark)
{
	const u64 n_tiles = ((u64)n_cand + 1 + LQ_FXSCAN_LINE_TILE - 1) / LQ_FXSCAN_LINE_TILE;
	for (u64 t = blockIdx.x; t < n_tiles; t += gridDim.x) {
		const u64 i64 = t * LQ_FXSCAN_LINE_TILE + threadIdx.x;
		if (i64 > n_cand) continue;
		const u32 i = (u32)i64;
		if (i == n_cand) { jump[i] = n_cand; mark[i] = 0; continue; }
		const u32 o = cand[i];
		uint4 lk; lk.x = lk.y = lk.z = lk.w = 0;
		u32 j = n_cand;
		if ((u64)o + 36 <= hi) {
			const u8 *p = base + o;
			u32 all = 0xff;
			for (u32 k = 0; k < 8; ++k) all &= p[4 + k] & p[24 + k];
			const u64 block_size = lq_bam_le32(p), l_name = p[12], n_cigar = (u64)p[16] | (u64)p[17] << 8, l_seq = lq_bam_le32(p + 20);
			const u64 fields = 32 + l_name + 4 * n_cigar + (l_seq + 1) / 2 + l_seq, next = (u64)o + 4 + block_size;
			if (all == 0xff && l_name >= 1 && l_seq <= 0x7fffffffULL && block_size <= 0x7fffffffULL && block_size >= fields && next <= hi
			    && p[36 + l_name - 1] == 0) {
				lk.x = (u32)next; lk.y = (u32)l_seq | 0x80000000u; lk.z = o + 36 + (u32)l_name + 4 * (u32)n_cigar;
				u32 a = i + 1, b = n_cand;                            // the first candidate at or behind next(o)
				while (a < b) { const u32 mid = a + (b - a) / 2; if (cand[mid] >= (u32)next) b = mid; else a = mid + 1; }
				if (next < hi && a < n_cand && cand[a] == (u32)next) j = a;
			}
		}
		lk.w = j;
		link[i] = lk; jump[i] = j; mark[i] = i == 0;
	}
}

// phase 0: cols[c][t] = records, segments, bases of candidate tile t.  phase 1 (cols scanned): rows[r], info[r] of every vouched record
// r of the chain in file order, positions relative to `org`; its segment in sseg and in qseg (with_qual: the quality bytes behind the
// packed sequence, else LQ_GATHER_FILL) if it has bases; resume[0] = the first chain element that is not vouched, or hi, relative to
// `org`.
static __global__ void __launch_bounds__(LQ_FXSCAN_THREADS)
k_bam_emit(const u8 *base, u32 org, const u32 *cand, u32 n_cand, const uint4 *link, const u32 *mark, u64 *cols, int phase, int with_qual,
           FxRow *rows, FxInfo *info, GatherSeg *sseg, GatherSeg *qseg, u32 *resume)
{
	__shared__ u64 wsum[LQ_FXSCAN_THREADS / 64];
	const u64 n_tiles = ((u64)n_cand + LQ_FXSCAN_LINE_TILE - 1) / LQ_FXSCAN_LINE_TILE;
	for (u64 t = blockIdx.x; t < n_tiles; t += gridDim.x) {
		const u64 i64 = t * LQ_FXSCAN_LINE_TILE + threadIdx.x;
		const u32 i = (u32)i64;
		const bool on = i64 < n_cand && mark[i];
		uint4 lk; lk.x = lk.y = lk.z = lk.w = 0;
		if (on) lk = link[i];
		const bool rec = lk.y >> 31;
		const u32 len = lk.y & 0x7fffffffu;
		// one scan for the three counts: a tile has 256 candidates (10 bits each for records and segments) of fewer than 2^31 bases
		u64 tot;
		const u64 e0 = lq_fx_block_scan(rec ? (u64)1 | (u64)(len ? 1 : 0) << 10 | (u64)len << 20 : 0, wsum, &tot);
		if (!phase) {
			if (threadIdx.x == 0) { cols[0 * n_tiles + t] = tot & 0x3ff; cols[1 * n_tiles + t] = tot >> 10 & 0x3ff; cols[2 * n_tiles + t] = tot >> 20; }
			continue;
		}
		if (!on) continue;
		const u32 o = cand[i];
		if (!rec) { resume[0] = o - org; continue; }              // (the chain ends at the first element that is not vouched)
		const u64 r = cols[0 * n_tiles + t] + (e0 & 0x3ff);
		FxInfo f;
		f.line = i; f.brk = 0; f.qend = 0; f.sseg = f.qseg = (u32)(cols[1 * n_tiles + t] + (e0 >> 10 & 0x3ff));
		f.has_qual = with_qual ? 1 : 0; f.dst = cols[2 * n_tiles + t] + (e0 >> 20);
		info[r] = f;
		const u32 at = o + 36;                                    // the name: up to its first NUL (there is one in front of the sequence)
		u32 q = at;
		while (base[q]) ++q;
		FxRow row; row.name_at = at - org; row.name_len = q - at; row.seq_len = len; row.flags = f.has_qual;
		rows[r] = row;
		if (len) {
			GatherSeg g; g.src = lk.z - org; g.dst = f.dst;
			sseg[f.sseg] = g;
			g.src = with_qual ? g.src + (len + 1) / 2 : LQ_GATHER_FILL;
			qseg[f.qseg] = g;
		}
		if (lk.w >= n_cand) resume[0] = lk.x - org;            // the last vouched record: what follows is no candidate, or the range's end
	}
}
