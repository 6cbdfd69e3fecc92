// longqc_amd/csrc/kernels_csv.hpp -- a comma-separated table with one header line read into typed columns on the device: the step in
// front of what lq_rs.run_platformqc (lq_rs.py:93-222) computes from the *.sts.csv of an RS-II run, where the reference calls
// pd.read_table(sep=',').  The host side is csv.cpp, the caller longqc_amd/rs.py; DESIGN 8 (21) has the domain and the float rule.
//
// A piece is a range of whole lines, each ending in '\n' (the host cuts it there and reads the header line itself).  Everything is
// parallel over bytes, over rows or over (row, wanted column) pairs; nothing walks the file.
//   k_csv_marks    per byte: cm[i] = 1 for ',', nl[i] = 1 for a '\n' that ends a line which is not empty (pandas skips "" and "\r").  The
//                  first byte outside the domain -- '"', NUL, a '\r' that no '\n' follows -- by atomicMin on its offset.
//   (the scans)    Prim::exclusive_scan over nl and cm (kernels_isort.hpp), n + 1 entries: rws[i] is the row of byte i, cmb[i] - cmb[the
//                  row's first byte] its field.
//   k_csv_rows     at the first byte of every row: rowat[row] = i, rowcm[row] = cmb[i].
//   k_csv_starts   at every ',' and every row-ending '\n': the field that ends here and the field that begins behind it, scattered into
//                  fbeg / fend (rows x wanted) where the field is a wanted one.  A '\r' before the '\n' is not part of the last field.  A
//                  row whose field count is not the header's: atomicMin on the offset of its first byte.
//   k_csv_parse    one lane per (row, wanted column): an int64 "[+-]?[0-9]{1,18}" or a double "[+-]?" digits, optional '.', digits
//                  with at most 15 significant digits and 22 decimals, whose value is ONE IEEE division of the exact integer mantissa by
//                  the exact power of ten (Clinger's fast path: correctly rounded, which is float(text)).  No fused arithmetic, no
//                  reciprocal: LQ_CSV_DIV is __ddiv_rn.  Every other field is flagged for the host twin (csv.cpp), which reads a number by
//                  strtod and refuses the rest with the line; the device never guesses.
// The statistics on the resident columns (lqcsv_lengths):
//   k_csv_lengths  per row len[i] = end[i] - start[i] as uint32 (outside 0 .. 2^32-1: counted, the call fails) and flag[i] = score[i] > t.
//   k_csv_pack     under the scanned flags: the lengths and the base counts compacted, the descending sort key ~len, sum / min / max
//                  of both by a block reduction and one atomic each per block.
//   N50 / N90      k_pol_unkey and k_pol_nxx of kernels_polread.hpp as they are: the same rule on the same kind of array.
#pragma once
#include "kernels_polread.hpp"

#define LQ_CSV_THREADS 256
#define LQ_CSV_MAX_BLOCKS 256u        // bytes / rows / pairs are strided over the blocks of a launch: 65536 a round
#define LQ_CSV_MAX_WANT 16            // wanted columns of a handle
#define LQ_CSV_INT_DIGITS 18          // an int64 field: 1 .. 18 digits
#define LQ_CSV_SIG_DIGITS 15          // a double field: significant digits (the mantissa stays below 2^53)
#define LQ_CSV_DECIMALS 22            // ... and digits behind the point (10^22 is the last exact power of ten)
#define LQ_CSV_MAX_BYTES 0xfffffe00u  // positions in a piece are 32-bit
#define LQ_CSV_NONE 0xffffffffffffffffULL
static_assert(LQ_CSV_THREADS == LQ_FXSCAN_THREADS, "lq_fx_block_scan scans a block of LQ_FXSCAN_THREADS");

#ifndef LQ_EMU
#define LQ_CSV_DIV(a, b) __ddiv_rn((a), (b))
#else
#define LQ_CSV_DIV(a, b) ((a) / (b))
#endif

struct CsvWant { u32 n, n_fields; u32 field[LQ_CSV_MAX_WANT]; u32 kind[LQ_CSV_MAX_WANT]; void *out[LQ_CSV_MAX_WANT]; };
struct CsvSums { unsigned long long sum_hq, min_hq, max_hq, sum_nb, min_nb, max_nb, n_range; };

// ctl words of a piece (the host sets them): 0 the first byte outside the domain, 1 the first byte of the first ragged row (both
// LQ_CSV_NONE), 2 the fields left to the host twin
static __global__ void __launch_bounds__(LQ_CSV_THREADS)
k_csv_marks(const u8 *d, u64 n, u32 *nl, u32 *cm, unsigned long long *ctl)
{
	for (u64 i = (u64)blockIdx.x * LQ_CSV_THREADS + threadIdx.x; i <= n; i += (u64)gridDim.x * LQ_CSV_THREADS) {
		if (i == n) { nl[i] = cm[i] = 0; continue; }              // (the scans run over n + 1 entries)
		const u32 c = d[i], p1 = i ? d[i - 1] : '\n', p2 = i > 1 ? d[i - 2] : '\n';
		const bool empty = p1 == '\n' || (p1 == '\r' && p2 == '\n');
		nl[i] = c == '\n' && !empty ? 1u : 0u;
		cm[i] = c == ',' ? 1u : 0u;
		if (c == '"' || c == 0 || (c == '\r' && (i + 1 >= n || d[i + 1] != '\n'))) atomicMin(ctl, (unsigned long long)i);
	}
}

// the first byte of a line that is not empty
__device__ __forceinline__ bool lq_csv_row_start(const u8 *d, u64 n, u64 i)
{
	if (i && d[i - 1] != '\n') return false;
	const u32 c = d[i];
	return c != '\n' && !(c == '\r' && i + 1 < n && d[i + 1] == '\n');
}

static __global__ void __launch_bounds__(LQ_CSV_THREADS)
k_csv_rows(const u8 *d, u64 n, const u32 *rws, const u32 *cmb, u32 n_rows, u32 *rowat, u32 *rowcm)
{
	for (u64 i = (u64)blockIdx.x * LQ_CSV_THREADS + threadIdx.x; i < n; i += (u64)gridDim.x * LQ_CSV_THREADS) {
		if (!lq_csv_row_start(d, n, i)) continue;
		const u32 r = rws[i];
		if (r < n_rows) { rowat[r] = (u32)i; rowcm[r] = cmb[i]; }
	}
}

__device__ __forceinline__ void lq_csv_put(const CsvWant &w, u32 field, u32 r, u32 *table, u32 v)
{
	for (u32 k = 0; k < w.n; ++k) if (w.field[k] == field) table[(u64)r * w.n + k] = v;
}

static __global__ void __launch_bounds__(LQ_CSV_THREADS)
k_csv_starts(const u8 *d, u64 n, const u32 *rws, const u32 *cmb, const u32 *rowat, const u32 *rowcm, u32 n_rows, CsvWant w, u32 *fbeg, u32 *fend,
             unsigned long long *ctl)
{
	for (u64 i = (u64)blockIdx.x * LQ_CSV_THREADS + threadIdx.x; i < n; i += (u64)gridDim.x * LQ_CSV_THREADS) {
		const u32 c = d[i], r = rws[i];
		if (r >= n_rows) continue;                                // (the empty lines behind the last row)
		if (lq_csv_row_start(d, n, i)) lq_csv_put(w, 0, r, fbeg, (u32)i);
		const bool row_end = c == '\n' && rws[i + 1] != r;
		if (c != ',' && !row_end) continue;
		const u32 f = cmb[i] - rowcm[r];                          // the field that ends at this byte
		lq_csv_put(w, f, r, fend, (u32)i - (row_end && i && d[i - 1] == '\r' ? 1u : 0u));
		if (!row_end) lq_csv_put(w, f + 1, r, fbeg, (u32)i + 1);
		else if (f + 1 != w.n_fields) atomicMin(ctl + 1, (unsigned long long)rowat[r]);
	}
}

#ifndef LQ_EMU
static __device__ const double lq_csv_pow10[LQ_CSV_DECIMALS + 1] =
#else
static const double lq_csv_pow10[LQ_CSV_DECIMALS + 1] =
#endif
	{ 1e0, 1e1, 1e2, 1e3, 1e4, 1e5, 1e6, 1e7, 1e8, 1e9, 1e10, 1e11, 1e12, 1e13, 1e14, 1e15, 1e16, 1e17, 1e18, 1e19, 1e20, 1e21, 1e22 };

// p[b .. e) = "[+-]?[0-9]{1,18}" -> true and its value
__device__ __forceinline__ bool lq_csv_int(const u8 *p, u32 b, u32 e, i64 *out)
{
	bool neg = false;
	if (b < e && (p[b] == '+' || p[b] == '-')) { neg = p[b] == '-'; ++b; }
	if (e <= b || e - b > LQ_CSV_INT_DIGITS) return false;
	u64 v = 0;
	for (u32 q = b; q < e; ++q) {
		const u32 c = (u32)p[q] - '0';
		if (c > 9) return false;
		v = v * 10 + c;
	}
	*out = neg ? -(i64)v : (i64)v;
	return true;
}

// p[b .. e) = "[+-]?" digits, optional '.', digits (a digit somewhere), at most LQ_CSV_SIG_DIGITS digits from the first that is not 0
// and at most LQ_CSV_DECIMALS behind the point -> true and the correctly rounded double
__device__ __forceinline__ bool lq_csv_double(const u8 *p, u32 b, u32 e, double *out)
{
	bool neg = false, point = false;
	if (b < e && (p[b] == '+' || p[b] == '-')) { neg = p[b] == '-'; ++b; }
	u64 m = 0;
	u32 sig = 0, dec = 0, digits = 0;
	for (u32 q = b; q < e; ++q) {
		const u32 c = p[q];
		if (c == '.') { if (point) return false; point = true; continue; }
		const u32 v = c - '0';
		if (v > 9) return false;
		++digits; dec += point ? 1u : 0u;
		if (m || v) ++sig;
		if (sig > LQ_CSV_SIG_DIGITS || dec > LQ_CSV_DECIMALS) return false;
		m = m * 10 + v;
	}
	if (!digits) return false;
	const double x = LQ_CSV_DIV((double)m, lq_csv_pow10[dec]);
	*out = neg ? -x : x;
	return true;
}

// column k of row row0 + r gets its value; flags[pair] = 1 and a zero value where the host twin has to read the field
static __global__ void __launch_bounds__(LQ_CSV_THREADS)
k_csv_parse(const u8 *d, u64 n, const u32 *fbeg, const u32 *fend, u32 n_rows, CsvWant w, u64 row0, u8 *flags, unsigned long long *ctl)
{
	const u64 n_pairs = (u64)n_rows * w.n;
	u32 n_host = 0;
	for (u64 p = (u64)blockIdx.x * LQ_CSV_THREADS + threadIdx.x; p < n_pairs; p += (u64)gridDim.x * LQ_CSV_THREADS) {
		const u32 k = (u32)(p % w.n);
		const u64 r = p / w.n;
		const u32 b = fbeg[p], e = fend[p];
		bool ok = b <= e && e <= n;                               // (always, for rows of the header's field count)
		if (w.kind[k] == 0) {
			i64 v = 0;
			ok = ok && lq_csv_int(d, b, e, &v);
			((i64*)w.out[k])[row0 + r] = ok ? v : 0;
		} else {
			double v = 0.0;
			ok = ok && lq_csv_double(d, b, e, &v);
			((double*)w.out[k])[row0 + r] = ok ? v : 0.0;
		}
		flags[p] = ok ? 0 : 1;
		n_host += ok ? 0u : 1u;
	}
	if (n_host) atomicAdd(ctl + 2, (unsigned long long)n_host);
}

// flag has n + 1 entries; *n_range counts the rows whose end - start lies outside 0 .. 2^32-1 (their len is 0)
static __global__ void __launch_bounds__(LQ_CSV_THREADS)
k_csv_lengths(const i64 *start, const i64 *end, const double *score, double threshold, u64 n, u32 *len, u32 *flag, unsigned long long *n_range)
{
	for (u64 i = (u64)blockIdx.x * LQ_CSV_THREADS + threadIdx.x; i <= n; i += (u64)gridDim.x * LQ_CSV_THREADS) {
		if (i == n) { flag[i] = 0; continue; }
		const i64 s = start[i], e = end[i];
		const u64 diff = (u64)e - (u64)s;                         // (e >= s: the true difference, which fits 64 bits)
		const bool bad = e < s || diff > 0xffffffffULL;
		len[i] = bad ? 0u : (u32)diff;
		flag[i] = score[i] > threshold ? 1u : 0u;
		if (bad) atomicAdd(n_range, 1ULL);
	}
}

// pos: the exclusive scan of flag.  The host sets sums to {0, ~0, 0, 0, ~0, 0, 0}
static __global__ void __launch_bounds__(LQ_CSV_THREADS)
k_csv_pack(const u32 *len, const i64 *bases, const u32 *flag, const u32 *pos, u64 n, u32 *hq32, u32 *nb32, u32 *key, CsvSums *sums)
{
	__shared__ u64 wsum[LQ_CSV_THREADS / 64];
	u64 sh = 0, hmin = LQ_U64MAX, hmax = 0, sb = 0, bmin = LQ_U64MAX, bmax = 0, nr = 0;
	for (u64 i = (u64)blockIdx.x * LQ_CSV_THREADS + threadIdx.x; i < n; i += (u64)gridDim.x * LQ_CSV_THREADS) {
		if (!flag[i]) continue;
		const u32 at = pos[i];
		const i64 b64 = bases[i];
		const bool bad = b64 < 0 || b64 > 0xffffffffLL;
		const u64 h = len[i], b = bad ? 0 : (u64)b64;
		nr += bad ? 1 : 0;
		hq32[at] = (u32)h; nb32[at] = (u32)b; key[at] = ~(u32)h;
		sh += h; hmin = h < hmin ? h : hmin; hmax = h > hmax ? h : hmax;
		sb += b; bmin = b < bmin ? b : bmin; bmax = b > bmax ? b : bmax;
	}
	for (int o = 1; o < 64; o <<= 1) {                            // (every lane of the block is here: the loop above has no collective)
		const u64 a = __shfl_xor(hmin, o), b = __shfl_xor(hmax, o), c = __shfl_xor(bmin, o), e = __shfl_xor(bmax, o);
		hmin = a < hmin ? a : hmin; hmax = b > hmax ? b : hmax; bmin = c < bmin ? c : bmin; bmax = e > bmax ? e : bmax;
	}
	u64 sh_all, sb_all, nr_all;
	lq_fx_block_scan(sh, wsum, &sh_all);
	lq_fx_block_scan(sb, wsum, &sb_all);
	lq_fx_block_scan(nr, wsum, &nr_all);
	if ((threadIdx.x & 63) == 0 && hmin <= hmax) {
		atomicMin(&sums->min_hq, (unsigned long long)hmin); atomicMax(&sums->max_hq, (unsigned long long)hmax);
		atomicMin(&sums->min_nb, (unsigned long long)bmin); atomicMax(&sums->max_nb, (unsigned long long)bmax);
	}
	if (threadIdx.x == 0) {
		if (sh_all) atomicAdd(&sums->sum_hq, (unsigned long long)sh_all);
		if (sb_all) atomicAdd(&sums->sum_nb, (unsigned long long)sb_all);
		if (nr_all) atomicAdd(&sums->n_range, (unsigned long long)nr_all);
	}
}
