// longqc_amd/csrc/kernels_dust_table.hpp -- the low-complexity table's rows as text, made on the device (dust.cpp: lqsdust_format,
// lqchunk_sdust_table): what the reference's `sdust` prints per read (sdust.c:211-217),
//   name '\t' masked '\t' len '\t' %.3f of masked/len '\t' %.3f of meanQ '\t' q7 '\n'        name_len + fields + 6 bytes
// from the arrays the scan left on the device.  About 60 bytes per read, a ten-thousandth of the chunk: one lane per row in every
// kernel, rows strided over a capped grid, no LDS, digits built in registers and stored byte by byte.
//   k_sdust_rows   per row: the two doubles (IEEE division, device log10), each reduced to a class and a count of thousandths by
//                  lq_fmt3_round (lq_fmt3.hpp: exactly what glibc's printf rounds to), the fields' widths and the row's bytes; the rows
//                  whose meanQ the device does not vouch for (below), the reads on LongQC's exclusion lists (longQC.py:370-371, on the
//                  printed fraction) and the chunk's integer sums through integer atomics -- no float reduction order exists.
//   k_sdust_patch  the host's meanQ for the unvouched rows (libm and the same rounding) over the device's entries.
//   k_sdust_text   the bytes, at the rows' starts (the engine's scan of the rows' byte counts, k_scan_lookback).
// Vouching: the device's log10 and glibc's are both within a few ulp of the true value but not bit-equal, so a row's meanQ text can
// differ only where z * 1000 lies within that error of k + 0.5.  A row is unvouched when |frac(|z| * 1000) - 0.5| < window * max(|z| *
// 1000, 1), window 2^-30 unless the caller says otherwise: 2^22 ulp of z * 1000 (DESIGN 8 has the two libraries' bounds).  A value
// that is not finite, or 2^50 or more, is unvouched too.  Without qualities no log is taken (0.0 / 0: "-nan") and nothing is to vouch.
#pragma once
#include "lq_common.hpp"
#include "lq_fmt3.hpp"
#include <cmath>

#define LQ_DTAB_THREADS 256
#define LQ_DTAB_MAX_BLOCKS 256u      // rows are strided over the blocks of a launch
#define LQ_DTAB_WINDOW 9.313225746154785e-10      // 2^-30

// meta[i]: the classes (LQ_F3_*) of the fraction (bits 0-3) and of meanQ (4-7), the bytes of their fields (8-15, 16-23)
#define LQ_DTAB_META(fc, qc, fw, qw) ((fc) | (qc) << 4 | (fw) << 8 | (qw) << 16)
// st[]: the launch's counters, zeroed before it
enum { LQ_DTAB_ST_UNV = 0, LQ_DTAB_ST_EX1, LQ_DTAB_ST_EX2, LQ_DTAB_ST_MASKED, LQ_DTAB_ST_Q7, LQ_DTAB_ST_WORDS = 8 };

struct alignas(16) DustUnv { u32 idx, len; double psum; };          // an unvouched row: what the host needs to take its meanQ
struct alignas(16) DustPatch { u64 qthou; u32 idx, qcls; };         // the host's answer

__device__ __forceinline__ u64 lq_dtab_put_u(u8 *out, u64 p, u64 v)
{
	const u32 nd = lq_ndigits(v);
	for (u32 k = nd; k-- > 0;) { out[p + k] = (u8)('0' + v % 10); v /= 10; }
	return p + nd;
}

__device__ __forceinline__ u64 lq_dtab_put_f3(u8 *out, u64 p, u32 cls, u64 thou)
{
	if (LQ_F3_CLASS(cls) == LQ_F3_NAN) { out[p] = '-'; out[p + 1] = 'n'; out[p + 2] = 'a'; out[p + 3] = 'n'; return p + 4; }
	if (cls & LQ_F3_NEG) out[p++] = '-';
	if (LQ_F3_CLASS(cls) == LQ_F3_INF) { out[p] = 'i'; out[p + 1] = 'n'; out[p + 2] = 'f'; return p + 3; }
	p = lq_dtab_put_u(out, p, thou / 1000u);
	const u32 f = (u32)(thou % 1000u);
	out[p] = '.'; out[p + 1] = (u8)('0' + f / 100); out[p + 2] = (u8)('0' + f / 10 % 10); out[p + 3] = (u8)('0' + f % 10);
	return p + 4;
}

// Row i: masked[i], q7[i], psum[i]; its length len[i], or off[i + 1] - off[i] with len == NULL; it has qualities if it has bases and
// has_q[i] != 0, or -- has_q == NULL -- the chunk has a quality buffer (qual != NULL) whose byte at the read's first base is not zero
// (sdust._rows' rule).  rbytes has n + 1 entries for the scan; the caller zeroes the last.  unv, ex1, ex2: room for n entries each.
__global__ void __launch_bounds__(LQ_DTAB_THREADS)
k_sdust_rows(u32 n, const u32 *nlen, const u32 *masked, const u32 *len, const u64 *off, const double *psum, const u8 *has_q, const u8 *qual,
             const u32 *q7, double window, u64 *fthou, u64 *qthou, u32 *meta, u32 *rbytes, DustUnv *unv, u32 *ex1, u32 *ex2,
             unsigned long long *st)
{
	u64 s_masked = 0, s_q7 = 0;
	for (u64 i = (u64)blockIdx.x * LQ_DTAB_THREADS + threadIdx.x; i < n; i += (u64)gridDim.x * LQ_DTAB_THREADS) {
		const u32 ln = len ? len[i] : (u32)(off[i + 1] - off[i]), mk = masked[i], q = q7[i];
		const bool hq = ln > 0 && (has_q ? has_q[i] != 0 : (qual != nullptr && qual[off[i]] != 0));
		u64 ft, qt = 0;
		const u32 fc = lq_fmt3_round((double)mk / (double)ln, &ft);
		u32 qc = LQ_F3_NAN;                                       // 0.0 / 0 without qualities
		if (hq) {
			const double ps = psum[i], z = -10 * log10(ps / (double)ln);
			qc = lq_fmt3_round(z, &qt);
			bool u = LQ_F3_CLASS(qc) != LQ_F3_FINITE;
			if (!u) { const double t = fabs(z) * 1000.0; u = fabs(t - floor(t) - 0.5) < window * fmax(t, 1.0); }
			if (u) { const u32 k = (u32)atomicAdd(st + LQ_DTAB_ST_UNV, 1ULL); unv[k].idx = (u32)i; unv[k].len = ln; unv[k].psum = ps; }
		}
		if (fc == LQ_F3_FINITE) {                                 // (a "-nan" row is on neither list)
			if (ln > 500000u && ft > 200) ex1[(u32)atomicAdd(st + LQ_DTAB_ST_EX1, 1ULL)] = (u32)i;
			if (ln > 10000u && ft > 400) ex2[(u32)atomicAdd(st + LQ_DTAB_ST_EX2, 1ULL)] = (u32)i;
		}
		const u32 fw = lq_fmt3_width(fc, ft), qw = lq_fmt3_width(qc, qt);
		fthou[i] = ft; qthou[i] = qt; meta[i] = LQ_DTAB_META(fc, qc, fw, qw);
		rbytes[i] = nlen[i] + lq_ndigits(mk) + lq_ndigits(ln) + fw + qw + lq_ndigits(q) + 6;
		s_masked += mk; s_q7 += q;
	}
	// every lane of the wave is here: one pair of atomics per wave
#pragma unroll
	for (int o = 32; o > 0; o >>= 1) { s_masked += __shfl_xor(s_masked, o); s_q7 += __shfl_xor(s_q7, o); }
	if ((threadIdx.x & 63) == 0 && (s_masked | s_q7)) {
		atomicAdd(st + LQ_DTAB_ST_MASKED, (unsigned long long)s_masked);
		atomicAdd(st + LQ_DTAB_ST_Q7, (unsigned long long)s_q7);
	}
}

__global__ void __launch_bounds__(LQ_DTAB_THREADS)
k_sdust_patch(u32 k, const DustPatch *pt, u64 *qthou, u32 *meta, u32 *rbytes)
{
	for (u64 j = (u64)blockIdx.x * LQ_DTAB_THREADS + threadIdx.x; j < k; j += (u64)gridDim.x * LQ_DTAB_THREADS) {
		const DustPatch p = pt[j];
		const u32 m = meta[p.idx], qw = lq_fmt3_width(p.qcls, p.qthou);
		qthou[p.idx] = p.qthou;
		meta[p.idx] = (m & 0xff0fu) | p.qcls << 4 | qw << 16;
		rbytes[p.idx] = rbytes[p.idx] - (m >> 16 & 0xffu) + qw;
	}
}

// the two fraction columns as the thousandths the text shows (lqchunk_sdust_columns), after k_sdust_patch: "-nan" as 0xffffffff /
// INT32_MIN, the sign of the text on meanQ ("-0.000" is 0).  *bad |= 1 for a meanQ that is infinite or does not fit 31 bits
__global__ void __launch_bounds__(LQ_DTAB_THREADS)
k_sdust_columns(u32 n, const u64 *fthou, const u64 *qthou, const u32 *meta, u32 *frac, i32 *qv, u32 *bad)
{
	for (u64 i = (u64)blockIdx.x * LQ_DTAB_THREADS + threadIdx.x; i < n; i += (u64)gridDim.x * LQ_DTAB_THREADS) {
		const u32 m = meta[i], fc = m & 0xfu, qc = m >> 4 & 0xfu;
		const u64 ft = fthou[i], qt = qthou[i];
		u32 f = 0xffffffffu; i32 q = (i32)0x80000000;
		bool err = false;
		if (LQ_F3_CLASS(fc) != LQ_F3_NAN) { err = LQ_F3_CLASS(fc) != LQ_F3_FINITE || ft >= 0xffffffffULL; f = (u32)ft; }
		if (LQ_F3_CLASS(qc) != LQ_F3_NAN) { err = err || LQ_F3_CLASS(qc) != LQ_F3_FINITE || qt >= 0x7fffffffULL; q = qc & LQ_F3_NEG ? -(i32)qt : (i32)qt; }
		if (err) atomicOr(bad, 1u);
		frac[i] = f; qv[i] = q;
	}
}

// rec[i]: the text byte at which row i starts.  names: row i's name at names[noff[i] .. noff[i] + nlen[i])
__global__ void __launch_bounds__(LQ_DTAB_THREADS)
k_sdust_text(u32 n, const u8 *names, const u64 *noff, const u32 *nlen, const u32 *masked, const u32 *len, const u64 *off, const u32 *q7,
             const u64 *fthou, const u64 *qthou, const u32 *meta, const u64 *rec, u8 *out)
{
	for (u64 i = (u64)blockIdx.x * LQ_DTAB_THREADS + threadIdx.x; i < n; i += (u64)gridDim.x * LQ_DTAB_THREADS) {
		u64 p = rec[i];
		const u32 nl = nlen[i], m = meta[i];
		const u8 *nm = names + noff[i];
		for (u32 k = 0; k < nl; ++k) out[p + k] = nm[k];
		p += nl;
		out[p++] = '\t';
		p = lq_dtab_put_u(out, p, masked[i]);
		out[p++] = '\t';
		p = lq_dtab_put_u(out, p, len ? len[i] : (u32)(off[i + 1] - off[i]));
		out[p++] = '\t';
		p = lq_dtab_put_f3(out, p, m & 0xfu, fthou[i]);
		out[p++] = '\t';
		p = lq_dtab_put_f3(out, p, m >> 4 & 0xfu, qthou[i]);
		out[p++] = '\t';
		p = lq_dtab_put_u(out, p, q7[i]);
		out[p] = '\n';
	}
}
