// longqc_amd/csrc/kernels_fxscan.hpp -- the record scan of the file reader's device mode (reader.cpp, lqreader_parse): the records of a
// range of FASTA/FASTQ bytes that lie on the device, found there, and the GatherSeg lists k_chunk_gather (kernels_gather.hpp) takes,
// written there.  The grammar is kseq's as reader.cpp::parse_one states it; the scan answers only for records it can vouch for
// (DESIGN 8 (13) has the domain) and names the state from which parse_one goes on.
//
// Everything is parallel over bytes or over lines; nothing walks the records one after the other.
//   k_fx_lines       a streaming pass over the bytes, 16 per lane and load: counts per tile (phase 0), and after k_fx_tilescan has
//                    made them offsets, the table of lines (phase 1).  Line i starts at L4[i].x; with its start the table keeps what
//                    lies in front of it: the marker bytes ('@', '>'), the lines whose first byte is '@', '>' or '+', the lines of two
//                    or more bytes that end in '\r' (kseq drops that byte), the lines the device leaves to the host (a line that is
//                    exactly "\r", an empty line after a line that ends in "\r\r") and the empty lines.  Every question about a run of
//                    lines -- its bytes without line breaks and dropped '\r', whether it is clean, where the next marker is -- is a
//                    difference of two entries or a bisection on one column.
//   k_fx_candidates  one lane per line that starts with '@' or '>', under the hypothesis that a record starts there: the end of the
//                    sequence (the next line that starts with '+', '>' or '@'), the last line of the quality string (a bisection on the
//                    lengths), whether the device vouches for the record, and the line where the next record would start.
//   k_fx_jump        the true records are the candidates reachable from the range's first header: pointer jumping, one launch per
//                    doubling, marks the path.
//   k_fx_emit        counts (phase 0), then the 16-byte row of every vouched record in file order (phase 1) and one GatherSeg per line
//                    that gives bytes (phase 2, one lane per line).
//   k_fx_tilescan    the exclusive scan of the per-tile counts (one block; a piece has a few thousand tiles).
//   k_fx_names       the names of the vouched records as the chunk keeps them -- each followed by one NUL, and n + 1 offsets -- and the
//                    first row whose name holds a byte of 0x80 or more: with them the host needs no byte of a vouched record
//                    (lqreader_host_copy).  Counts per tile of rows (phase 0), k_fx_tilescan, the copy (phase 1).
//   k_fx_rebase, k_fx_tileseg   the reader's and lq_chunk_gather's: segments moved into a chunk's lists, the gather's per-tile table.
// Grids are capped and the tiles strided over the blocks, as in every chunk-step kernel.  LDS: one word per wave for the block scans.
#pragma once
#include "chunk.hpp"

#define LQ_FXSCAN_THREADS 256
#define LQ_FXSCAN_TILE 4096u          // bytes of one (block, round) of k_fx_lines: 256 lanes x 16 bytes
#define LQ_FXSCAN_LINE_TILE 256u      // lines of one (block, round) of k_fx_candidates, k_fx_jump and k_fx_emit
#define LQ_FXSCAN_MAX_BLOCKS 1024u    // tiles are strided over the blocks of a launch
#define LQ_FXSCAN_TILESEG_MAX_BLOCKS 4u   // k_fx_tileseg: one lane per gather tile, a bisection each
#define LQ_FXSCAN_LINE_COLS 6         // k_fx_lines' counts per tile: line breaks, markers, break lines, dropped '\r', host lines, empty lines
#define LQ_FXSCAN_EMIT_COLS 4         // k_fx_emit's: records, sequence segments, quality segments, bases
#define LQ_FXSCAN_MAX_BYTES 0xffffff00u   // positions are 32-bit

struct alignas(16) FxRow { u32 name_at, name_len, seq_len, flags; };    // flags bit 0: the record has a quality string
struct alignas(16) FxInfo { u32 line, brk, qend, sseg; u32 qseg, has_qual; u64 dst; };      // a vouched record: header line, '+' / next header line, last quality line; its first segments, its first base

__device__ __forceinline__ bool lq_fx_marker(u32 c) { return c == '@' || c == '>'; }
__device__ __forceinline__ bool lq_fx_space(u32 c) { return c == ' ' || (c >= 9 && c <= 13); }

// exclusive scan of v over the block (every thread calls it); *total: the block's sum.  wsum: LQ_FXSCAN_THREADS / 64 words of LDS
__device__ __forceinline__ u64 lq_fx_block_scan(u64 v, u64 *wsum, u64 *total)
{
	const u32 lane = threadIdx.x & 63, w = threadIdx.x >> 6;
	u64 inc = v;
	for (u32 d = 1; d < 64; d <<= 1) {
		const u64 t = __shfl_up(inc, d);
		if (lane >= d) inc += t;
	}
	if (lane == 63) wsum[w] = inc;
	__syncthreads();
	u64 base = 0, tot = 0;
	for (u32 i = 0; i < LQ_FXSCAN_THREADS / 64; ++i) { const u64 s = wsum[i]; if (i < w) base += s; tot += s; }
	__syncthreads();                                          // (wsum serves the next call)
	*total = tot;
	return base + inc - v;
}

// cols: n_cols columns of n_tiles counts -> their exclusive prefix sums, totals[c] the sum of column c
static __global__ void __launch_bounds__(LQ_FXSCAN_THREADS)
k_fx_tilescan(u64 *cols, u64 n_tiles, u32 n_cols, u64 *totals)
{
	__shared__ u64 wsum[LQ_FXSCAN_THREADS / 64];
	for (u32 c = 0; c < n_cols; ++c) {
		u64 *col = cols + (u64)c * n_tiles, carry = 0;
		for (u64 b = 0; b < n_tiles; b += LQ_FXSCAN_THREADS) {
			const u64 i = b + threadIdx.x;
			const u64 v = i < n_tiles ? col[i] : 0;
			u64 tot;
			const u64 ex = lq_fx_block_scan(v, wsum, &tot);
			if (i < n_tiles) col[i] = carry + ex;
			carry += tot;
		}
		if (threadIdx.x == 0) totals[c] = carry;
	}
}

// base: the bytes, 16-byte aligned; the range is base[lo .. hi), lo the first byte of a line.  Tile t is base[(lo & ~15) + 4096 t ..).
// phase 0: cols[c][t] = the tile's count of column c.  phase 1 (cols scanned, totals[] the sums): L4[i] = {start of line i, markers,
// break lines, dropped '\r' in front of it}, L2[i] = {host lines, empty lines in front of it}, for i = 0 .. n_lines with n_lines =
// totals[0] + 1 (the last line is the one without a line break, possibly empty; entry n_lines: start hi + 1 and the sums).
static __global__ void __launch_bounds__(LQ_FXSCAN_THREADS, 8)       // (eight waves per SIMD: a streaming pass)
k_fx_lines(const u8 *base, u32 lo, u32 hi, u64 n_tiles, u64 *cols, const u64 *totals, int phase, uint4 *L4, uint2 *L2)
{
	__shared__ u64 wsum[LQ_FXSCAN_THREADS / 64];
	const u32 t0 = lo & ~15u;
	if (phase && blockIdx.x == 0 && threadIdx.x == 0) {
		uint4 a; a.x = lo; a.y = a.z = a.w = 0;
		uint2 b; b.x = b.y = 0;
		L4[0] = a; L2[0] = b;
		const u64 nl = totals[0] + 1;
		a.x = hi + 1; a.y = (u32)totals[1]; a.z = (u32)totals[2]; a.w = (u32)totals[3];
		b.x = (u32)totals[4]; b.y = (u32)totals[5];
		L4[nl] = a; L2[nl] = b;
	}
	for (u64 t = blockIdx.x; t < n_tiles; t += gridDim.x) {
		const u64 w64 = (u64)t0 + t * LQ_FXSCAN_TILE + (u64)threadIdx.x * 16;
		const u32 w0 = (u32)w64;
		const bool live = w64 < hi;
		uint4 v; v.x = v.y = v.z = v.w = 0;
		u32 prev = 0x0a0a0a0au;                                   // the three bytes in front of the word; what lies in front of lo counts as a line break
		if (live) {
			v = *(const uint4*)(base + w0);
			if (w0 >= 4) prev = *(const u32*)(base + w0 - 4);
		}
		u32 c1 = w0 >= lo + 1 ? prev >> 24 : '\n', c2 = w0 >= lo + 2 ? (prev >> 16 & 255) : '\n', c3 = w0 >= lo + 3 ? (prev >> 8 & 255) : '\n';
		u32 n_nl = 0, n_a = 0, n_b = 0, n_d = 0, n_x = 0, n_e = 0;
		// the lane's counts first; phase 1 then takes their prefix and walks the word again, storing at every line break
		#pragma unroll 1
		for (u32 k = 0; k < 16; ++k) {
			const u32 p = w0 + k;
			const u32 word = k < 8 ? (k < 4 ? v.x : v.y) : (k < 12 ? v.z : v.w);
			u32 c = word >> (8 * (k & 3)) & 255;
			const bool in = live && p >= lo && p < hi;
			if (!in) c = '\n';
			if (in) {
				const bool mk = lq_fx_marker(c);
				n_a += mk;
				n_b += c1 == '\n' && (mk || c == '+');
				if (c == '\n') {
					++n_nl;
					n_d += c1 == '\r' && c2 != '\n';
					n_x += (c1 == '\r' && c2 == '\n') || (c1 == '\n' && c2 == '\r' && c3 == '\r');
					n_e += c1 == '\n';
				}
			}
			c3 = c2; c2 = c1; c1 = c;
		}
		const u64 b0 = (u64)n_nl | (u64)n_a << 16 | (u64)n_b << 32 | (u64)n_d << 48;      // (a tile has 4096 bytes: 16 bits hold every count)
		const u64 b1 = (u64)n_x | (u64)n_e << 16;
		u64 tot0, tot1;
		const u64 e0 = lq_fx_block_scan(b0, wsum, &tot0), e1 = lq_fx_block_scan(b1, wsum, &tot1);
		if (!phase) {
			if (threadIdx.x == 0) {
				cols[0 * n_tiles + t] = tot0 & 0xffff; cols[1 * n_tiles + t] = tot0 >> 16 & 0xffff; cols[2 * n_tiles + t] = tot0 >> 32 & 0xffff;
				cols[3 * n_tiles + t] = tot0 >> 48; cols[4 * n_tiles + t] = tot1 & 0xffff; cols[5 * n_tiles + t] = tot1 >> 16 & 0xffff;
			}
			continue;
		}
		if (!n_nl) continue;
		// what lies in front of this lane's word
		u32 g_nl = (u32)(cols[0 * n_tiles + t] + (e0 & 0xffff)), g_a = (u32)(cols[1 * n_tiles + t] + (e0 >> 16 & 0xffff));
		u32 g_b = (u32)(cols[2 * n_tiles + t] + (e0 >> 32 & 0xffff)), g_d = (u32)(cols[3 * n_tiles + t] + (e0 >> 48));
		u32 g_x = (u32)(cols[4 * n_tiles + t] + (e1 & 0xffff)), g_e = (u32)(cols[5 * n_tiles + t] + (e1 >> 16 & 0xffff));
		c1 = w0 >= lo + 1 ? prev >> 24 : '\n'; c2 = w0 >= lo + 2 ? (prev >> 16 & 255) : '\n'; c3 = w0 >= lo + 3 ? (prev >> 8 & 255) : '\n';
		#pragma unroll 1
		for (u32 k = 0; k < 16; ++k) {
			const u32 p = w0 + k;
			const u32 word = k < 8 ? (k < 4 ? v.x : v.y) : (k < 12 ? v.z : v.w);
			u32 c = word >> (8 * (k & 3)) & 255;
			const bool in = p >= lo && p < hi;
			if (!in) c = '\n';
			if (in) {
				const bool mk = lq_fx_marker(c);
				g_a += mk;
				g_b += c1 == '\n' && (mk || c == '+');
				if (c == '\n') {
					++g_nl;
					g_d += c1 == '\r' && c2 != '\n';
					g_x += (c1 == '\r' && c2 == '\n') || (c1 == '\n' && c2 == '\r' && c3 == '\r');
					g_e += c1 == '\n';
					uint4 a; a.x = p + 1; a.y = g_a; a.z = g_b; a.w = g_d;
					uint2 b; b.x = g_x; b.y = g_e;
					L4[g_nl] = a; L2[g_nl] = b;
				}
			}
			c3 = c2; c2 = c1; c1 = c;
		}
	}
}

// the first line k >= from whose entry k + 1 of column y (markers) / z (break lines) exceeds v: the first line at or behind `from` that
// holds a marker / starts with '@', '>' or '+'; n_lines if there is none
__device__ __forceinline__ u32 lq_fx_next_marker(const uint4 *L4, u32 from, u32 n_lines, u32 v)
{
	u32 a = from, b = n_lines;
	while (a < b) { const u32 mid = a + (b - a) / 2; if (L4[mid + 1].y > v) b = mid; else a = mid + 1; }
	return a;
}
__device__ __forceinline__ u32 lq_fx_next_break(const uint4 *L4, u32 from, u32 n_lines, u32 v)
{
	u32 a = from, b = n_lines;
	while (a < b) { const u32 mid = a + (b - a) / 2; if (L4[mid + 1].z > v) b = mid; else a = mid + 1; }
	return a;
}
// the first byte of line i, 0 for an empty line
__device__ __forceinline__ u32 lq_fx_first(const u8 *base, const uint4 *L4, u32 i) { const u32 s = L4[i].x; return L4[i + 1].x - 1 > s ? base[s] : 0; }

// cand[i] = {the line where the record behind this one starts (n_lines: none), the line that ends the sequence, the last quality
// line, sequence length | has a quality string << 31}; .y == 0: line i starts no record the device vouches for.  jump[i] = cand[i].x
// for such a record, else n_lines; jump[n_lines] = n_lines.  mark[i] = 1 for the range's first header line, else 0.  hdr0: 0, or the
// header character in front of the range -- line 0 is then the rest of a header line.
static __global__ void __launch_bounds__(LQ_FXSCAN_THREADS)
k_fx_candidates(const u8 *base, const uint4 *L4, const uint2 *L2, u32 n_lines, u32 hdr0, uint4 *cand, u32 *jump, u32 *mark)
{
	const u64 n_tiles = ((u64)n_lines + 1 + LQ_FXSCAN_LINE_TILE - 1) / LQ_FXSCAN_LINE_TILE;
	for (u64 t = blockIdx.x; t < n_tiles; t += gridDim.x) {
		const u64 i64 = t * LQ_FXSCAN_LINE_TILE + threadIdx.x;
		if (i64 > n_lines) continue;
		const u32 i = (u32)i64;
		if (i == n_lines) { jump[i] = n_lines; mark[i] = 0; continue; }
		uint4 cd; cd.x = n_lines; cd.y = cd.z = cd.w = 0;
		const u32 c = hdr0 && i == 0 ? hdr0 : lq_fx_first(base, L4, i);      // (hdr0: the parser has consumed the header character of line 0)
		u32 is_start = 0;
		if (lq_fx_marker(c)) {
			const uint4 h = L4[i], s = L4[i + 1];                 // (s: the first line behind the header)
			is_start = hdr0 ? i == 0 : h.y == 0;                      // no marker in front of this line
			const u32 m = lq_fx_next_break(L4, i + 1, n_lines, s.z);
			if (m < n_lines && L2[m].x == L2[i + 1].x) {              // the sequence ends inside the range, and none of its lines is the host's
				const uint4 lm = L4[m];
				const u32 len = (lm.x - s.x) - (m - i - 1) - (lm.w - s.w);
				if (len < 0x80000000u) {
					if (base[lm.x] != '+') { cd.x = m; cd.y = m; cd.z = m; cd.w = len; }
					else if (m + 2 < n_lines) {                       // (the '+' line and one line behind it end in a line break)
						const uint4 q = L4[m + 1];
						// the first line e whose end brings the quality string to len bytes or more; lines up to n_lines - 2 end in a line break
						u32 a = m + 1, b = n_lines - 1;
						while (a < b) {
							const u32 mid = a + (b - a) / 2;
							const uint4 x = L4[mid + 1];
							if ((x.x - q.x) - (mid - m) - (x.w - q.w) >= len) b = mid; else a = mid + 1;
						}
						if (a < n_lines - 1) {
							const uint4 x = L4[a + 1];
							if ((x.x - q.x) - (a - m) - (x.w - q.w) == len && L2[a + 1].x == L2[m + 1].x) {
								const u32 k = lq_fx_next_marker(L4, a + 1, n_lines, x.y);
								cd.x = k < n_lines && lq_fx_marker(lq_fx_first(base, L4, k)) ? k : n_lines;
								cd.y = m; cd.z = a; cd.w = len | 0x80000000u;
							}
						}
					}
				}
			}
		}
		cand[i] = cd;
		jump[i] = cd.y ? cd.x : n_lines;
		mark[i] = is_start;
	}
}

// one doubling: what a marked line points at is marked, and every line points twice as far
static __global__ void __launch_bounds__(LQ_FXSCAN_THREADS)
k_fx_jump(const u32 *jin, u32 *jout, u32 *mark, u32 n_lines)
{
	const u64 n_tiles = ((u64)n_lines + 1 + LQ_FXSCAN_LINE_TILE - 1) / LQ_FXSCAN_LINE_TILE;
	for (u64 t = blockIdx.x; t < n_tiles; t += gridDim.x) {
		const u64 i = t * LQ_FXSCAN_LINE_TILE + threadIdx.x;
		if (i > n_lines) continue;
		const u32 j = jin[i];
		if (j < n_lines && mark[i]) mark[j] = 1;
		jout[i] = jin[j];
	}
}

// phase 0: cols[c][t] = records, sequence segments, quality segments, bases of line tile t.  phase 1 (cols scanned): rows[r], info[r]
// of every vouched record r in file order, positions relative to `org`; qseg of a record without a quality string; resume[0 .. 2) =
// position and last_char behind the last vouched record.  phase 2: sseg / qseg of every line that gives bytes.
static __global__ void __launch_bounds__(LQ_FXSCAN_THREADS, 8)       // (eight waves per SIMD: a streaming pass)
k_fx_emit(const u8 *base, u32 org, const uint4 *L4, const uint2 *L2, u32 n_lines, u32 hdr0, const uint4 *cand, const u32 *mark, u64 *cols, int phase,
          FxRow *rows, FxInfo *info, GatherSeg *sseg, GatherSeg *qseg, u32 *resume)
{
	__shared__ u64 wsum[LQ_FXSCAN_THREADS / 64];
	const u64 n_tiles = ((u64)n_lines + LQ_FXSCAN_LINE_TILE - 1) / LQ_FXSCAN_LINE_TILE;
	for (u64 t = blockIdx.x; t < n_tiles; t += gridDim.x) {
		const u64 i64 = t * LQ_FXSCAN_LINE_TILE + threadIdx.x;
		const u32 i = (u32)i64;
		const bool live = i64 < n_lines;
		uint4 cd; cd.x = cd.y = cd.z = cd.w = 0;
		bool rec = false;
		if (live && mark[i]) { cd = cand[i]; rec = cd.y != 0; }
		const u32 m = cd.y, e = cd.z, len = cd.w & 0x7fffffffu;
		const bool has_qual = cd.w >> 31;
		u64 tot;
		if (phase == 2) {
			const u64 before = lq_fx_block_scan(rec ? 1 : 0, wsum, &tot) + cols[0 * n_tiles + t] + (rec ? 1 : 0);
			if (!live || before == 0) continue;
			const FxInfo f = info[before - 1];
			const uint4 l = L4[i];
			if (L4[i + 1].x - 1 == l.x) continue;                     // an empty line gives no bytes
			if (i > f.line && i < f.brk) {
				const uint4 s = L4[f.line + 1];
				GatherSeg g; g.src = l.x - org; g.dst = f.dst + ((l.x - s.x) - (i - f.line - 1) - (l.w - s.w));
				sseg[f.sseg + (i - f.line - 1) - (L2[i].y - L2[f.line + 1].y)] = g;
			} else if (f.has_qual && i > f.brk && i <= f.qend) {
				const uint4 s = L4[f.brk + 1];
				GatherSeg g; g.src = l.x - org; g.dst = f.dst + ((l.x - s.x) - (i - f.brk - 1) - (l.w - s.w));
				qseg[f.qseg + (i - f.brk - 1) - (L2[i].y - L2[f.brk + 1].y)] = g;
			}
			continue;
		}
		u32 n_ss = 0, n_qs = 0;
		if (rec) {
			n_ss = (m - i - 1) - (L2[m].y - L2[i + 1].y);
			n_qs = has_qual ? (e - m) - (L2[e + 1].y - L2[m + 1].y) : len ? 1 : 0;
		}
		const u64 e0 = lq_fx_block_scan((u64)(rec ? 1 : 0) | (u64)n_ss << 32, wsum, &tot);
		u64 tot_q, tot_d;
		const u64 eq = lq_fx_block_scan(n_qs, wsum, &tot_q), ed = lq_fx_block_scan(rec ? len : 0, wsum, &tot_d);
		if (!phase) {
			if (threadIdx.x == 0) {
				cols[0 * n_tiles + t] = tot & 0xffffffffu; cols[1 * n_tiles + t] = tot >> 32; cols[2 * n_tiles + t] = tot_q; cols[3 * n_tiles + t] = tot_d;
			}
			continue;
		}
		if (!rec) continue;
		const u64 r = cols[0 * n_tiles + t] + (e0 & 0xffffffffu);
		FxInfo f;
		f.line = i; f.brk = m; f.qend = e; f.sseg = (u32)(cols[1 * n_tiles + t] + (e0 >> 32)); f.qseg = (u32)(cols[2 * n_tiles + t] + eq);
		f.has_qual = has_qual; f.dst = cols[3 * n_tiles + t] + ed;
		info[r] = f;
		const u32 at = L4[i].x + (hdr0 && i == 0 ? 0 : 1), end = L4[i + 1].x - 1;            // the name: up to the first space character of the header line
		u32 q = at;
		while (q < end && !lq_fx_space(base[q])) ++q;
		FxRow row; row.name_at = at - org; row.name_len = q - at; row.seq_len = len; row.flags = has_qual;
		rows[r] = row;
		if (!has_qual && len) { GatherSeg g; g.src = LQ_GATHER_FILL; g.dst = f.dst; qseg[f.qseg] = g; }
		if (cd.x >= n_lines || cand[cd.x].y == 0) {                   // the last vouched record
			const u32 at2 = has_qual ? L4[e + 1].x : L4[m].x + 1;
			resume[0] = at2 - org; resume[1] = has_qual ? 0 : base[L4[m].x];
		}
	}
}

// d: the bytes the rows' positions count from.  phase 0: cols[t] = the bytes of tile t's names, a NUL behind each; *first_bad = n_rows.
// phase 1 (cols scanned): names[name_off[i] ..) = the name of row i and a NUL, name_off[n_rows] = the blob's length; *first_bad = the
// first row whose name holds a byte of 0x80 or more.  One lane per row: a name is a few tens of bytes.
static __global__ void __launch_bounds__(LQ_FXSCAN_THREADS, 8)
k_fx_names(const u8 *d, const FxRow *rows, u64 n_rows, u64 *cols, int phase, char *names, u64 *name_off, unsigned long long *first_bad)
{
	__shared__ u64 wsum[LQ_FXSCAN_THREADS / 64];
	if (!phase && blockIdx.x == 0 && threadIdx.x == 0) *first_bad = n_rows;
	const u64 n_tiles = (n_rows + LQ_FXSCAN_LINE_TILE - 1) / LQ_FXSCAN_LINE_TILE;
	for (u64 t = blockIdx.x; t < n_tiles; t += gridDim.x) {
		const u64 i = t * LQ_FXSCAN_LINE_TILE + threadIdx.x;
		const bool live = i < n_rows;
		u32 at = 0, len = 0;
		if (live) { const FxRow w = rows[i]; at = w.name_at; len = w.name_len; }
		u64 tot;
		const u64 ex = lq_fx_block_scan(live ? (u64)len + 1 : 0, wsum, &tot);
		if (!phase) { if (threadIdx.x == 0) cols[t] = tot; continue; }
		if (!live) continue;
		const u64 o = cols[t] + ex;
		name_off[i] = o;
		if (i + 1 == n_rows) name_off[n_rows] = o + len + 1;
		const u8 *src = d + at;
		u32 high = 0;
		for (u32 k = 0; k < len; ++k) { const u8 c = src[k]; names[o + k] = (char)c; high |= c; }
		names[o + len] = 0;
		if (high & 0x80) atomicMin(first_bad, (unsigned long long)i);
	}
}

// out[i] = in[i] moved by (src_add, dst_add); a segment without source bytes keeps LQ_GATHER_FILL
static __global__ void __launch_bounds__(LQ_FXSCAN_THREADS)
k_fx_rebase(const GatherSeg *in, u64 n, u64 src_add, u64 dst_add, GatherSeg *out)
{
	for (u64 i = (u64)blockIdx.x * LQ_FXSCAN_THREADS + threadIdx.x; i < n; i += (u64)gridDim.x * LQ_FXSCAN_THREADS) {
		GatherSeg g = in[i];
		if (g.src != LQ_GATHER_FILL) g.src += src_add;
		g.dst += dst_add;
		out[i] = g;
	}
}

// k_chunk_gather's work list from segments that lie on the device: tile_seg[t] = the last segment s with segs[s].dst <= tile * t,
// tile_seg[n_tiles] = n_segs - 1 (segs: n_segs entries in destination order, the first at 0)
static __global__ void __launch_bounds__(LQ_FXSCAN_THREADS)
k_fx_tileseg(const GatherSeg *segs, u32 n_segs, u64 n_tiles, u32 tile, u32 *tile_seg)
{
	for (u64 t = (u64)blockIdx.x * LQ_FXSCAN_THREADS + threadIdx.x; t <= n_tiles; t += (u64)gridDim.x * LQ_FXSCAN_THREADS) {
		if (t == n_tiles) { tile_seg[t] = n_segs - 1; continue; }
		const u64 d = t * tile;
		u32 a = 0, b = n_segs - 1;
		while (a < b) { const u32 mid = a + (b - a + 1) / 2; if (segs[mid].dst <= d) a = mid; else b = mid - 1; }
		tile_seg[t] = a;
	}
}
