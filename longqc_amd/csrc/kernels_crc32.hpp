// longqc_amd/csrc/kernels_crc32.hpp -- the CRC-32 of RFC 1952 (reflected polynomial 0xEDB88320, zlib's crc32(0, buf, len)) of byte
// ranges of a buffer that lies on the device: what lets the file reader check a gzip member without its bytes coming back to the
// host (reader.cpp, lqreader_host_copy).
//
// A unit is a range of at most LQ_CRC_UNIT bytes (a BGZF member is at most that long); the host cuts longer ranges into units and
// merges their values with zlib's crc32_combine (CrcDev).  One wave per unit and workgroup, units strided over a capped grid.  The
// register of a CRC is affine in its start value and linear in the message, so:
//   * the unit's bytes are read as aligned 16-byte words; what lies in front of its first byte in the first word counts as zeros,
//     which a register that starts at zero does not see;
//   * the start value 0xFFFFFFFF is the complement of the message's first four bytes (units of less than four bytes: byte by byte);
//   * the words are dealt out from the back: lane 63 takes the last 64 full words, lane 62 the 64 in front of them ..., so every
//     lane stands for LQ_CRC_SHARE bytes (the first ones: zeros) and the merge needs constants only: in step k a lane's value is
//     multiplied by x^(8 * LQ_CRC_SHARE * 2^k) mod P and the value 2^k lanes behind it is added, six steps for the wave;
//   * the bytes behind the last full word (less than 16) go through the merged register one by one.
// A lane's own pass is slicing-by-8: eight tables of 256 words that the workgroup makes in LDS (8 KiB), two steps per 16-byte word.
// Only the aligned words that hold bytes of a range are read.  With one wave per workgroup the tables limit a CU to 20 waves; the
// registers (under 64 VGPRs) would admit 32.
#pragma once
#include "chunk.hpp"
#include <zlib.h>
#include <vector>

#define LQ_CRC_THREADS 64             // one wave per workgroup: a unit is one wave's
#define LQ_CRC_UNIT 65536u            // bytes of one unit at most: 64 lanes x LQ_CRC_SHARE
#define LQ_CRC_SHARE 1024u            // bytes one lane stands for: 64 words of 16
#define LQ_CRC_MAX_BLOCKS 1024u       // units are strided over the workgroups of a launch
#define LQ_CRC_POLY 0xEDB88320u

struct alignas(16) CrcUnit { u64 off; u32 len, pad; };        // bytes[off .. off + len), len <= LQ_CRC_UNIT

// a * b mod P, both in the reflected form (bit 31 is x^0)
__host__ __device__ constexpr inline u32 lq_crc_mulmod(u32 a, u32 b)
{
	u32 p = 0;
	for (int i = 0; i < 32; ++i) {
		p ^= (a >> (31 - i) & 1) ? b : 0;
		b = (b >> 1) ^ ((b & 1) ? LQ_CRC_POLY : 0);
	}
	return p;
}
// x^(2^n) mod P
__host__ __device__ constexpr inline u32 lq_crc_x2n(int n)
{
	u32 p = 0x40000000u;                                      // x^1
	for (int i = 0; i < n; ++i) p = lq_crc_mulmod(p, p);
	return p;
}

// the bytes of a 32-bit word, which holds the word's positions p0 .. p0 + 3, whose position lies in [lo, hi): 0xff each
__device__ __forceinline__ u32 lq_crc_mask(i64 p0, i64 lo, i64 hi)
{
	u32 m = 0;
	for (int k = 0; k < 4; ++k) if (p0 + k >= lo && p0 + k < hi) m |= 0xffu << (8 * k);
	return m;
}

// word `at` (positions at .. at + 15 of the unit's aligned bytes) as the register sees it: zeros in front of the first byte `head`,
// the first four bytes of the message complemented
__device__ __forceinline__ uint4 lq_crc_fix(uint4 v, i64 at, i64 head)
{
	v.x = (v.x & lq_crc_mask(at, head, at + 16)) ^ lq_crc_mask(at, head, head + 4);
	v.y = (v.y & lq_crc_mask(at + 4, head, at + 16)) ^ lq_crc_mask(at + 4, head, head + 4);
	v.z = (v.z & lq_crc_mask(at + 8, head, at + 16)) ^ lq_crc_mask(at + 8, head, head + 4);
	v.w = (v.w & lq_crc_mask(at + 12, head, at + 16)) ^ lq_crc_mask(at + 12, head, head + 4);
	return v;
}

// eight bytes (lo: the first four) through the register c.  T: the eight tables, T[k][b] the register after byte b and k zero bytes
__device__ __forceinline__ u32 lq_crc_step8(const u32 (*T)[256], u32 c, u32 lo, u32 hi)
{
	lo ^= c;
	return T[7][lo & 255] ^ T[6][lo >> 8 & 255] ^ T[5][lo >> 16 & 255] ^ T[4][lo >> 24] ^
	       T[3][hi & 255] ^ T[2][hi >> 8 & 255] ^ T[1][hi >> 16 & 255] ^ T[0][hi >> 24];
}

#define LQ_CRC_MERGE_STEP(k) { \
	constexpr u32 xk = lq_crc_x2n(13 + (k));                  /* x^(8 * 1024 * 2^k) */ \
	const u32 behind = __shfl_down(c, 1u << (k)); \
	c = lq_crc_mulmod(c, xk) ^ behind; }

// out[u] = crc32 of bytes[units[u].off .. + units[u].len) for u < n.  bytes + off may have any residue mod 16: the words are those of
// the address.  What a unit reads: the aligned 16-byte words that hold at least one of its bytes.
static __global__ void __launch_bounds__(LQ_CRC_THREADS)
k_crc32_ranges(const u8 *bytes, const CrcUnit *units, u32 n, u32 *out)
{
	__shared__ u32 T[8][256];
	for (u32 b = threadIdx.x; b < 256; b += LQ_CRC_THREADS) {
		u32 c = b;
		for (int k = 0; k < 8; ++k) c = (c >> 1) ^ ((c & 1) ? LQ_CRC_POLY : 0);
		T[0][b] = c;
	}
	__syncthreads();
	for (u32 b = threadIdx.x; b < 256; b += LQ_CRC_THREADS) {
		u32 c = T[0][b];
		for (int k = 1; k < 8; ++k) { c = (c >> 8) ^ T[0][c & 255]; T[k][b] = c; }
	}
	__syncthreads();
	const u32 lane = threadIdx.x;
	for (u64 u = blockIdx.x; u < n; u += gridDim.x) {
		const CrcUnit un = units[u];
		const u8 *first = bytes + un.off;
		if (un.len < 4) {                                         // (wave-uniform; the lanes all do the same)
			u32 c = 0xffffffffu;
			for (u32 k = 0; k < un.len; ++k) c = (c >> 8) ^ T[0][(c ^ first[k]) & 255];
			if (lane == 0) out[u] = ~c;
			continue;
		}
		const i64 head = (i64)((uintptr_t)first & 15);
		const u8 *a0 = first - head;
		const i64 total = head + (i64)un.len, W = total >> 4;    // the aligned bytes up to the range's end; their full words, at most 4096
		i64 w0 = W - (i64)(64 - lane) * 64, w1 = w0 + 64;
		if (w0 < 0) w0 = 0;
		u32 c = 0;
		#pragma unroll 2
		for (i64 w = w0; w < w1; ++w) {
			uint4 v = *(const uint4*)(a0 + w * 16);
			if (w < 2) v = lq_crc_fix(v, w * 16, head);
			c = lq_crc_step8(T, c, v.x, v.y);
			c = lq_crc_step8(T, c, v.z, v.w);
		}
		LQ_CRC_MERGE_STEP(0) LQ_CRC_MERGE_STEP(1) LQ_CRC_MERGE_STEP(2) LQ_CRC_MERGE_STEP(3) LQ_CRC_MERGE_STEP(4) LQ_CRC_MERGE_STEP(5)
		const u32 tail = (u32)(total & 15);
		if (lane == 0) {                                          // (lane 0 holds the merged register)
			if (tail) {
				uint4 v = *(const uint4*)(a0 + W * 16);
				if (W < 2) v = lq_crc_fix(v, W * 16, head);
				for (u32 k = 0; k < tail; ++k) {
					const u32 word = k < 8 ? (k < 4 ? v.x : v.y) : (k < 12 ? v.z : v.w);
					c = (c >> 8) ^ T[0][(c ^ (word >> (8 * (k & 3)))) & 255];
				}
			}
			out[u] = ~c;
		}
	}
}

// k_crc32_ranges over ranges the host names: ranges longer than a unit are cut and their values merged here
struct CrcDev {
	DBuf units, out;
	std::vector<CrcUnit> h_units; std::vector<u32> h_out;

	// crc_out[i] = crc32 of d_bytes[off[i] .. off[i] + len[i]); d_bytes on the device, readable up to the end of the aligned 16-byte
	// word of every range's last byte.  Waits for the stream.
	void run(hipStream_t stream, const u8 *d_bytes, u32 n, const u64 *off, const u64 *len, u32 *crc_out)
	{
		h_units.clear();
		for (u32 i = 0; i < n; ++i) {
			u64 o = off[i], l = len[i];
			do {
				const u32 m = (u32)std::min<u64>(l, LQ_CRC_UNIT);
				h_units.push_back({o, m, 0});
				o += m; l -= m;
			} while (l);
		}
		const u64 nu = h_units.size();
		if (!nu) return;
		if (nu > 0xffffffffULL) throw std::invalid_argument("more than 2^32-1 units of CRC32");
		units.ensure((size_t)nu * sizeof(CrcUnit)); out.ensure((size_t)nu * 4);
		h_out.resize((size_t)nu);
		LQ_HIP_CHECK(hipMemcpyAsync(units.p, h_units.data(), (size_t)nu * sizeof(CrcUnit), hipMemcpyHostToDevice, stream));
		const u32 grid = (u32)std::min<u64>(nu, LQ_CRC_MAX_BLOCKS);
		LQ_LAUNCH(k_crc32_ranges, grid, LQ_CRC_THREADS, stream, d_bytes, (const CrcUnit*)units.as<CrcUnit>(), (u32)nu, out.as<u32>());
		LQ_HIP_CHECK(hipGetLastError());
		LQ_HIP_CHECK(hipMemcpyAsync(h_out.data(), out.p, (size_t)nu * 4, hipMemcpyDeviceToHost, stream));
		LQ_HIP_CHECK(hipStreamSynchronize(stream));
		u64 k = 0;
		for (u32 i = 0; i < n; ++i) {
			u32 c = h_out[k]; u64 l = len[i];
			for (l -= h_units[k++].len; l; l -= h_units[k++].len) c = (u32)crc32_combine(c, h_out[k], (z_off_t)h_units[k].len);
			crc_out[i] = c;
		}
	}
};
