// longqc_amd/csrc/lq_fmt3.hpp -- a double as printf's "%.3f" prints it, reduced to a class, a sign and an integer count of
// thousandths: the one rounding rule of the low-complexity table's two fraction columns, for the device (kernels_dust_table.hpp) and
// for the host (dust.cpp: the rows the device does not vouch for, and lqsdust_main's loop).
//
// glibc converts exactly: the binary value x = m * 2^e (m < 2^53) is rounded to the nearest multiple of 1/1000, ties to even.  With
// |x| < 2^50 that needs 64-bit integers only: m * 1000 < 2^63; for e < 0 the count is (m * 1000) >> -e, rounded up when the bits
// shifted out exceed half a unit, or equal it with the count odd; a shift of 64 or more leaves less than half of one unit: 0.  A value
// of 2^50 or more is LQ_F3_BIG: neither column reaches it from 32-bit counts and finite doubles (masked / len <= 2^32, |10 log10| of
// a positive double < 3240), the caller refuses it.
#pragma once
#include <cstdint>
#include <cstring>

#if defined(__HIPCC__) || defined(LQ_EMU)
#define LQ_HD __host__ __device__
#else
#define LQ_HD
#endif

#define LQ_F3_FINITE 0u
#define LQ_F3_NAN    1u              // printed "-nan": the sign x86 gives 0.0 / 0 and keeps through log10 and the product
#define LQ_F3_INF    2u
#define LQ_F3_BIG    3u              // finite, 2^50 or more
#define LQ_F3_NEG    4u              // the sign bit, beside LQ_F3_FINITE (-0.0 prints "-0.000"), LQ_F3_INF and LQ_F3_BIG
#define LQ_F3_CLASS(c) ((c) & 3u)

// -> the class (with LQ_F3_NEG); *thou: the thousandths of |x| for LQ_F3_FINITE, else 0
LQ_HD inline uint32_t lq_fmt3_round(double x, uint64_t *thou)
{
	uint64_t b;
	memcpy(&b, &x, 8);
	const uint32_t neg = (b >> 63) ? LQ_F3_NEG : 0u, ex = (uint32_t)(b >> 52) & 0x7ffu;
	uint64_t m = b & ((1ULL << 52) - 1);
	*thou = 0;
	if (ex == 0x7ffu) return m ? LQ_F3_NAN : (LQ_F3_INF | neg);
	if (ex >= 1073u) return LQ_F3_BIG | neg;                  // |x| >= 2^50
	uint32_t s;                                               // x = m * 2^-s, s >= 3
	if (ex) { m |= 1ULL << 52; s = 1075u - ex; } else s = 1074u;
	if (s >= 64u) return LQ_F3_FINITE | neg;
	const uint64_t p = m * 1000u, r = p & ((1ULL << s) - 1), half = 1ULL << (s - 1);
	uint64_t q = p >> s;
	if (r > half || (r == half && (q & 1))) ++q;
	*thou = q;
	return LQ_F3_FINITE | neg;
}

LQ_HD inline uint32_t lq_ndigits(uint64_t v) { uint32_t n = 1; while (v >= 10) { v /= 10; ++n; } return n; }

// the bytes "%.3f" gives the value
LQ_HD inline uint32_t lq_fmt3_width(uint32_t cls, uint64_t thou)
{
	const uint32_t neg = (cls & LQ_F3_NEG) ? 1u : 0u;
	if (LQ_F3_CLASS(cls) == LQ_F3_NAN) return 4;
	if (LQ_F3_CLASS(cls) == LQ_F3_INF) return 3 + neg;
	return neg + lq_ndigits(thou / 1000u) + 4;
}
