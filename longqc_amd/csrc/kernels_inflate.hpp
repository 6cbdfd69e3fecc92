// longqc_amd/csrc/kernels_inflate.hpp -- k_bgzf_inflate: raw DEFLATE (RFC 1951) for a batch of BGZF members (bgzf.hpp), the opt-in
// second way to inflate a BAM or bgzip FASTA/FASTQ file (reader.cpp, lqreader_inflate).  A member is an independent deflate stream of
// at most 64 KiB whose input and output ranges the host knows before a byte is inflated, so a launch is a list of jobs.
//
// One wave per member, one wave per workgroup.  The symbol decode is serial and wave-uniform: every lane carries the same bit buffer
// and walks the same symbols; no lane waits for another.  What the wave does in parallel: the compressed bytes come in 256-byte
// chunks, one aligned word per lane, the next chunk requested while the current one is consumed, and the bit buffer takes its words
// from them by lane index; the code tables are built from the code lengths by ballots (counts and the canonical order) and filled one
// symbol per lane; a match is copied 64 bytes per step, lane i reading out[pos - dist + i % dist], so a distance below the length
// needs no second pass; stored blocks are copied 64 bytes per step from the input; the finished member goes to global memory in
// aligned 16-byte words.
//
// The 64-KiB history lives in LDS (with the tables 70 496 bytes per workgroup: two members per CU of 160 KiB, 2 waves per CU; the
// VGPR budget is not what limits it).  A copy reads bytes that other lanes of the wave stored: every copy is behind a workgroup
// barrier, which for a workgroup of one wave is the wait for the LDS operations before it.  The history is laid out at the
// destination's residue mod 16, so the write-out moves aligned words on both sides; the bytes in front of the first and behind the last
// whole word are written one by one: nothing outside [out, out + isize) is written.
//
// Decode tables: a 10-bit first-level table per alphabet (entry: code length << 9 | symbol, 0: not there) and, for the codes longer
// than that and for the bit patterns no code has, the canonical walk over the per-length counts and the symbols in code order.
//
// A corrupt member is an input: for any bytes the kernel reads only the aligned words that hold [in, in + in_len), writes only inside
// [out, out + isize), ends (every loop iteration consumes at least one bit of a finite input, or fails) and leaves a status:
//   LQ_INF_OK        the stream ended with its final block after exactly isize bytes
//   LQ_INF_INVALID   not a deflate stream: block type 3, LEN != ~NLEN, more than 286 / 30 codes, a code-length set that is
//                    over-subscribed or incomplete (but for a single code of one bit), no end-of-block code, a repeat without a
//                    length before it or past the last code, a bit pattern no code has, symbols 286, 287, distance codes 30, 31, a
//                    distance that reaches in front of the member's first byte
//   LQ_INF_INPUT     the input ended inside the stream (also "invalid": the stream is not whole)
//   LQ_INF_LONG      a valid stream so far that gives more than isize bytes
//   LQ_INF_SHORT     a valid stream that ended before isize bytes
// In the order zlib finds them: what is wrong with a token first, then the room for its bytes.
#pragma once
#include "lq_common.hpp"

#define LQ_INFLATE_THREADS 64
#define LQ_INFLATE_MAX_BLOCKS 512u   // members are strided over the workgroups of a launch: two per CU
#define LQ_INFLATE_PAD 16u           // bytes the compressed buffer extends past its last byte (the bit reader loads aligned words)
#define LQ_INF_FAST 10               // bits of the first-level tables

enum { LQ_INF_OK = 0, LQ_INF_INVALID = 1, LQ_INF_INPUT = 2, LQ_INF_LONG = 3, LQ_INF_SHORT = 4 };

// one member: its deflate bytes comp[in .. in + in_len), its inflated bytes out[out .. out + isize), isize <= 65536
struct alignas(8) InflateJob { u64 in, out; u32 in_len, isize; };

// the bit reader: wave-uniform but for the two chunk registers, which hold word (64 * chunk + lane) of the member's aligned words
struct LqBits {
	const u32 *words; u32 n_words;                            // the aligned words that hold the member's bytes
	u32 a0;                                                   // bytes of the first word in front of the member
	u32 cur, nxt;                                             // per lane: the chunk in use, the chunk after it
	u32 k;                                                    // the next word to take
	u64 bb; u32 bc;                                           // the bit buffer and its count
	u32 used, total;                                          // bits consumed, bits the member has (in_len < 2^24)
};

__device__ __forceinline__ u32 lq_inf_chunk(const LqBits &b, u32 c)
{
	const u32 i = c * 64 + (threadIdx.x & 63);
	return i < b.n_words ? b.words[i] : 0u;
}

__device__ __forceinline__ u32 lq_inf_word(LqBits &b)
{
	if ((b.k & 63) == 0) { b.cur = b.nxt; b.nxt = lq_inf_chunk(b, (b.k >> 6) + 1); }
	const u32 w = (u32)__builtin_amdgcn_readlane((int)b.cur, (int)(b.k & 63));
	++b.k;
	return w;
}

// the reader stands at byte `byte` of the member
__device__ __forceinline__ void lq_inf_seek(LqBits &b, u32 byte)
{
	const u32 ab = b.a0 + byte, k = ab >> 2, skip = (ab & 3) * 8;
	b.cur = lq_inf_chunk(b, k >> 6); b.nxt = lq_inf_chunk(b, (k >> 6) + 1);
	b.bb = (u64)((u32)__builtin_amdgcn_readlane((int)b.cur, (int)(k & 63)) >> skip);
	b.bc = 32 - skip; b.k = k + 1;
	b.used = byte * 8;
}

__device__ __forceinline__ void lq_inf_refill(LqBits &b)       // -> at least 33 bits in the buffer (zeros behind the last word)
{
	if (b.bc <= 32) { b.bb |= (u64)lq_inf_word(b) << b.bc; b.bc += 32; }
}

__device__ __forceinline__ u32 lq_inf_take(LqBits &b, u32 n)   // n <= 32 bits of the buffer
{
	const u32 v = (u32)(b.bb & (((u64)1 << n) - 1));
	b.bb >>= n; b.bc -= n; b.used += n;
	return v;
}

// The decode tables of one alphabet from the code lengths lens[0 .. n) (n <= 320): tab (1 << fast entries), the symbols in code order
// and the count per length.  strict: an incomplete set is refused whatever it is (the code-length alphabet); otherwise a single
// code of one bit passes.  -> 0, or LQ_INF_INVALID.  Wave-collective; ends behind a barrier.
__device__ __forceinline__ u32 lq_inf_build(const u8 *lens, u32 n, u32 fast, bool strict, u16 *tab, u16 *order, u16 *cnt)
{
	const u32 lane = threadIdx.x & 63;
	const u64 below = ((u64)1 << lane) - 1;
	__syncthreads();                                          // the lengths are written, nobody decodes with the old tables
	u32 c[16];
#pragma unroll
	for (int b = 0; b < 16; ++b) c[b] = 0;
	for (u32 base = 0; base < n; base += 64) {
		const u32 l = base + lane < n ? lens[base + lane] : 0u;
#pragma unroll
		for (int b = 1; b < 16; ++b) c[b] += (u32)__popcll(__ballot(l == (u32)b));
	}
	i32 left = 1; u32 max = 0;
#pragma unroll
	for (int b = 1; b < 16; ++b) { left = left * 2 - (i32)c[b]; if (left < 0) return LQ_INF_INVALID; if (c[b]) max = (u32)b; }
	if (left > 0 && max != 0 && (strict || max != 1)) return LQ_INF_INVALID;
	u32 offs[16], first[16];                                  // where a length's symbols begin in `order`; its first code
	offs[0] = offs[1] = 0; first[0] = first[1] = 0;
#pragma unroll
	for (int b = 1; b < 15; ++b) { offs[b + 1] = offs[b] + c[b]; first[b + 1] = (first[b] + c[b]) << 1; }
	for (u32 i = lane; i < (1u << fast); i += 64) tab[i] = 0;
#pragma unroll
	for (int b = 0; b < 16; ++b) if (lane == (u32)b) cnt[b] = (u16)c[b];
	__syncthreads();
	u32 run[16];
#pragma unroll
	for (int b = 0; b < 16; ++b) run[b] = 0;
	for (u32 base = 0; base < n; base += 64) {
		const u32 s = base + lane, l = s < n ? lens[s] : 0u;
		u32 idx = 0, code = 0;
#pragma unroll
		for (int b = 1; b < 16; ++b) {
			const u64 m = __ballot(l == (u32)b);
			if (l == (u32)b) { const u32 r = run[b] + (u32)__popcll(m & below); idx = offs[b] + r; code = first[b] + r; }
			run[b] += (u32)__popcll(m);
		}
		if (l) {
			order[idx] = (u16)s;
			if (l <= fast) {                                        // the stream holds a code from its highest bit on
				const u32 rev = __brev(code) >> (32 - l);
				for (u32 i = rev; i < (1u << fast); i += 1u << l) tab[i] = (u16)(l << 9 | s);
			}
		}
	}
	__syncthreads();
	return 0;
}

// one symbol from the buffer's low bits (at least 15 are there, zeros behind the input's end) -> the symbol, *len: its code's
// length; 0xffff: no code begins with these bits
__device__ __forceinline__ u32 lq_inf_symbol(const LqBits &b, u32 fast, const u16 *tab, const u16 *order, const u16 *cnt, u32 *len)
{
	const u32 e = tab[(u32)b.bb & ((1u << fast) - 1)];
	if (e) { *len = e >> 9; return e & 511; }
	u32 code = 0, first = 0, index = 0;
	for (u32 l = 1; l <= 15; ++l) {
		code |= (u32)(b.bb >> (l - 1)) & 1;
		const u32 count = cnt[l];
		if (code < first + count) { *len = l; return order[index + (code - first)]; }
		index += count; first = (first + count) << 1; code <<= 1;
	}
	*len = 15;
	return 0xffff;
}

// the order in which a dynamic block gives the lengths of the code-length alphabet (RFC 1951 3.2.7)
__device__ const u8 lq_inf_order19[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

// n_jobs members: comp: the compressed bytes, 4-byte aligned, LQ_INFLATE_PAD bytes allocated past the last; out: the destination,
// 16-byte aligned (a job's `out` is relative to it); status[j]: LQ_INF_*
__global__ void __launch_bounds__(LQ_INFLATE_THREADS)
k_bgzf_inflate(const u8 *comp, const InflateJob *jobs, u32 n_jobs, u8 *out, u32 *status)
{
	__shared__ uint4 hist[4096 + 1];                          // 64 KiB and the destination's residue mod 16
	__shared__ u16 tab_l[1 << LQ_INF_FAST], tab_d[1 << LQ_INF_FAST];
	__shared__ u16 order_l[288], order_d[32], cnt_l[16], cnt_d[16];
	__shared__ u8 lens[320], cl19[32];                        // the code lengths of both alphabets as one run; of the code-length alphabet
	const u32 lane = threadIdx.x & 63;
	for (u32 j = blockIdx.x; j < n_jobs; j += gridDim.x) {
		const InflateJob job = jobs[j];
		const u32 isize = job.isize < 65536 ? job.isize : 65536u, shift = (u32)(job.out & 15);
		u8 *h = (u8*)hist + shift;                                     // byte i of the member: h[i]
		LqBits b;
		b.a0 = (u32)(job.in & 3); b.words = (const u32*)(comp + (job.in & ~(u64)3)); b.n_words = (b.a0 + job.in_len + 3) >> 2;
		b.total = job.in_len * 8;
		lq_inf_seek(b, 0);
		u32 pos = 0, st = LQ_INF_OK, last = 0;
		while (!st && !last) {
			lq_inf_refill(b);
			last = lq_inf_take(b, 1);
			const u32 type = lq_inf_take(b, 2);
			if (b.used > b.total) { st = LQ_INF_INPUT; break; }
			if (type == 3) { st = LQ_INF_INVALID; break; }
			if (type == 0) {                                          // stored: LEN, ~LEN at the next byte border, then the bytes
				const u32 at = (b.used + 7) >> 3;
				if (at + 4 > job.in_len) { st = LQ_INF_INPUT; break; }
				lq_inf_seek(b, at);
				lq_inf_refill(b);
				const u32 v = lq_inf_take(b, 32), n = v & 0xffff;
				if ((v >> 16) != (n ^ 0xffff)) { st = LQ_INF_INVALID; break; }
				const u32 have = job.in_len - (at + 4);
				u32 m = n < have ? n : have;
				if (m > isize - pos) m = isize - pos;
				const u8 *src = comp + job.in + at + 4;
				for (u32 i = lane; i < m; i += 64) h[pos + i] = src[i];
				pos += m;
				if (m < n) { st = n > have ? LQ_INF_INPUT : LQ_INF_LONG; break; }
				lq_inf_seek(b, at + 4 + n);
				continue;
			}
			if (type == 1) {                                          // the fixed codes (RFC 1951 3.2.6)
				for (u32 i = lane; i < 320; i += 64) lens[i] = i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : i < 288 ? 8 : 5;
				lq_inf_build(lens, 288, LQ_INF_FAST, false, tab_l, order_l, cnt_l);
				lq_inf_build(lens + 288, 32, LQ_INF_FAST, false, tab_d, order_d, cnt_d);
			} else {
				const u32 nlen = lq_inf_take(b, 5) + 257, ndist = lq_inf_take(b, 5) + 1, ncode = lq_inf_take(b, 4) + 4;
				if (b.used > b.total) { st = LQ_INF_INPUT; break; }
				if (nlen > 286 || ndist > 30) { st = LQ_INF_INVALID; break; }
				__syncthreads();                                      // (nobody reads the lengths of the block before)
				if (lane < 19) cl19[lane] = 0;
				__syncthreads();
				for (u32 i = 0; i < ncode; ++i) {
					lq_inf_refill(b);
					const u32 l = lq_inf_take(b, 3);
					if (lane == 0) cl19[lq_inf_order19[i]] = (u8)l;
				}
				if (b.used > b.total) { st = LQ_INF_INPUT; break; }
				if (lq_inf_build(cl19, 19, 7, true, tab_l, order_l, cnt_l)) { st = LQ_INF_INVALID; break; }
				// the lengths of both alphabets are one run: a repeat may cross from the one into the other
				u32 i = 0, prev = 0;
				while (i < nlen + ndist) {
					lq_inf_refill(b);
					u32 cl;
					const u32 sym = lq_inf_symbol(b, 7, tab_l, order_l, cnt_l, &cl);
					if (sym == 0xffff) { st = b.total - b.used < 7 ? LQ_INF_INPUT : LQ_INF_INVALID; break; }
					lq_inf_take(b, cl);
					u32 rep = 1, val = sym;
					if (sym == 16) { if (i == 0) { st = LQ_INF_INVALID; break; } val = prev; rep = 3 + lq_inf_take(b, 2); }
					else if (sym == 17) { val = 0; rep = 3 + lq_inf_take(b, 3); }
					else if (sym == 18) { val = 0; rep = 11 + lq_inf_take(b, 7); }
					if (b.used > b.total) { st = LQ_INF_INPUT; break; }
					if (i + rep > nlen + ndist) { st = LQ_INF_INVALID; break; }
					if (lane == 0) for (u32 r = 0; r < rep; ++r) lens[i + r] = (u8)val;
					i += rep; prev = val;
				}
				if (st) break;
				__syncthreads();
				if (lens[256] == 0) { st = LQ_INF_INVALID; break; }           // no end-of-block code
				if (lq_inf_build(lens, nlen, LQ_INF_FAST, false, tab_l, order_l, cnt_l)) { st = LQ_INF_INVALID; break; }
				if (lq_inf_build(lens + nlen, ndist, LQ_INF_FAST, false, tab_d, order_d, cnt_d)) { st = LQ_INF_INVALID; break; }
			}
			for (;;) {                                                // the block's symbols
				lq_inf_refill(b);
				u32 cl;
				u32 sym = lq_inf_symbol(b, LQ_INF_FAST, tab_l, order_l, cnt_l, &cl);
				if (sym == 0xffff) { st = b.total - b.used < 15 ? LQ_INF_INPUT : LQ_INF_INVALID; break; }
				lq_inf_take(b, cl);
				if (b.used > b.total) { st = LQ_INF_INPUT; break; }
				if (sym < 256) {
					if (pos >= isize) { st = LQ_INF_LONG; break; }
					if (lane == 0) h[pos] = (u8)sym;
					++pos;
					continue;
				}
				if (sym == 256) break;
				if (sym > 285) { st = LQ_INF_INVALID; break; }
				sym -= 257;
				const u32 lx = sym < 8 || sym == 28 ? 0u : (sym - 4) >> 2;
				const u32 len = (sym < 8 ? sym + 3 : sym == 28 ? 258u : ((4 + (sym & 3)) << lx) + 3) + lq_inf_take(b, lx);
				if (b.used > b.total) { st = LQ_INF_INPUT; break; }
				lq_inf_refill(b);
				const u32 ds = lq_inf_symbol(b, LQ_INF_FAST, tab_d, order_d, cnt_d, &cl);
				if (ds == 0xffff) { st = b.total - b.used < 15 ? LQ_INF_INPUT : LQ_INF_INVALID; break; }
				lq_inf_take(b, cl);
				if (b.used > b.total) { st = LQ_INF_INPUT; break; }
				if (ds > 29) { st = LQ_INF_INVALID; break; }
				const u32 dx = ds < 4 ? 0u : (ds - 2) >> 1;
				const u32 dist = (ds < 4 ? ds + 1 : ((2 + (ds & 1)) << dx) + 1) + lq_inf_take(b, dx);
				if (b.used > b.total) { st = LQ_INF_INPUT; break; }
				if (dist > pos) { st = LQ_INF_INVALID; break; }
				const u32 m = len < isize - pos ? len : isize - pos;
				__syncthreads();                                      // the bytes stored so far, by whichever lane, are there
				const u8 *src = h + (pos - dist);
				if (dist >= m) for (u32 i = lane; i < m; i += 64) h[pos + i] = src[i];
				else for (u32 i = lane; i < m; i += 64) h[pos + i] = src[i % dist];
				pos += m;
				if (m < len) { st = LQ_INF_LONG; break; }
			}
		}
		if (!st && pos != isize) st = LQ_INF_SHORT;
		__syncthreads();
		// the member (what there is of it) to its place: single bytes up to the first 16-byte border and from the last one on
		u8 *dst = out + job.out;
		const u32 head = pos < ((16 - shift) & 15) ? pos : ((16 - shift) & 15), body = (pos - head) & ~15u;
		if (lane < head) dst[lane] = h[lane];
		for (u32 i = lane * 16; i < body; i += 64 * 16) *(uint4*)(dst + head + i) = *(const uint4*)(h + head + i);
		if (lane < pos - head - body) dst[head + body + lane] = h[head + body + lane];
		if (lane == 0) status[j] = st;
		__syncthreads();                                          // the history is free for the next member
	}
}
