// longqc_amd/csrc/kernels_adapt.hpp -- the adapter search of LongQC's sampleqc (lq_adapt.py:10-78): per read end, what
// `edlib.align(adapter, window, mode="HW", task="path")` reports -- the edit distance d, the first optimal end e, the start s
// edlib's reverse pass picks for it (the smallest one: "we want the longest alignment") and the length L of the path its
// traceback takes through the NW matrix of adapter x window[s..e].
//
// One wave per read end.  Lane i holds adapter row 64b + i + 1 of band b and sweeps the window along anti-diagonals: at
// step t it computes column j = t - i + 1 from its own previous cell (left), the cell lane i - 1 made one step earlier
// (up, one __shfl_up) and the one lane i - 1 made two steps earlier (diagonal, the previous shuffle's result).  Adapters of
// up to 64 bases are one band; longer ones run band after band, the last lane of a band leaving its row in LDS for lane 0
// of the next (the banded instantiation).  Both sweeps keep a cell in one word, the two 16-bit fields compared or read
// directly:
//   1. HW (row 0 free): D << 16 | S, S the smallest start of an optimal path into the cell.  The lexicographic minimum over
//      the three predecessors is the unsigned minimum of the words; the adapter's last row gives d, e (first column with the
//      minimum) and s.
//   2. NW over window[s..e]: D << 16 | L, L the length of edlib's traceback path to the cell -- 1 + L of the cell it steps
//      to: up if D(up) + 1 == D, else left if D(left) + 1 == D, else the diagonal.
// Cells compare bytes exactly (edlib: N and lower case match only themselves).  Limits (checked by the host): window length
// <= LQ_ADAPT_MAXLEN, adapter length <= LQ_ADAPT_MAXADP, so that every field fits 16 bits.
#pragma once
#include "lq_common.hpp"
#ifndef LQ_SHARED
#define LQ_SHARED __shared__
#endif

#define LQ_ADAPT_THREADS 64          // one wave = one read end at a time
#define LQ_ADAPT_MAXLEN 4096         // window length (LongQC: 150)
#define LQ_ADAPT_MAXADP 32768        // adapter length (LongQC's presets: 18-64)
#define LQ_ADAPT_MAX_BLOCKS 16384    // read ends are strided over the blocks of a launch

// out[4k .. 4k+3] = d, s, e, L of window k (the wlen bytes at seq + woff[k]: a read end inside the resident chunk) against adp[0..m);
// e = -1 (the whole adapter deleted) gives s = 0, L = m
template <bool BANDED>
__global__ void __launch_bounds__(LQ_ADAPT_THREADS)
k_adapt(const u8 *seq, const u64 *woff, u32 n_ends, u32 wlen, const u8 *adp, u32 m, i32 *out)
{
	LQ_SHARED u32 s_row[BANDED ? LQ_ADAPT_MAXLEN + 1 : 1];      // row 64b of the current band: the last row of the band before
	const i32 lane = (i32)threadIdx.x;
	const u32 n_bands = BANDED ? (m + 63) / 64 : 1;
	for (u32 k = blockIdx.x; k < n_ends; k += gridDim.x) {
		const u8 *w = seq + woff[k];
		// ---- sweep 1: HW, cells D << 16 | S ----
		u32 best = m << 16;                                  // row m, column 0 (e = -1, s = 0)
		i32 best_e = -1;
		const i32 last_lane = (i32)((m - 1) & 63);
		for (u32 b = 0; b < n_bands; ++b) {
			const u32 R = 64 * b + (u32)lane + 1;            // this lane's adapter row
			const u32 nrows = m - 64 * b < 64 ? m - 64 * b : 64;
			const bool row_on = R <= m;
			const u32 a = row_on ? adp[R - 1] : 0u;
			const bool keep_row = BANDED && b + 1 < n_bands && lane == 63;
			u32 cur = R << 16, prev_up = 0;                   // column 0: D = R, any path starts at 0
			const i32 n_steps = (i32)wlen + (i32)nrows - 1;
			for (i32 t = 0; t < n_steps; ++t) {
				const i32 j = t - lane + 1;
				const u32 up_l = __shfl_up(cur, 1);
				u32 up = up_l, dg = prev_up;
				if (lane == 0 && j >= 1 && j <= (i32)wlen) {
					if (b == 0) { up = (u32)j; dg = (u32)(j - 1); }          // row 0: D = 0, the path starts at column j
					else { up = s_row[j]; dg = j == 1 ? (R - 1) << 16 : s_row[j - 1]; }
				}
				if (row_on && j >= 1 && j <= (i32)wlen) {
					const u32 c = a != w[j - 1];
					const u32 ul = (up < cur ? up : cur) + (1u << 16);
					const u32 dd = dg + (c << 16);
					cur = dd < ul ? dd : ul;
					if (keep_row) s_row[j] = cur;
					if (R == m && (cur >> 16) < (best >> 16)) { best = cur; best_e = j - 1; }
				}
				prev_up = up_l;
			}
			if (BANDED) __syncthreads();                      // (one wave per block: orders the row's LDS words for lane 0)
		}
		best = (u32)__builtin_amdgcn_readlane((int)best, last_lane);
		best_e = __builtin_amdgcn_readlane(best_e, last_lane);
		const i32 d = (i32)(best >> 16), s = (i32)(best & 0xffffu);
		// ---- sweep 2: NW over window[s..e], cells D << 16 | L ----
		i32 L = (i32)m;
		if (best_e >= 0) {
			const u8 *w2 = w + s;
			const i32 W2 = best_e - s + 1;
			u32 fin = 0;
			for (u32 b = 0; b < n_bands; ++b) {
				const u32 R = 64 * b + (u32)lane + 1;
				const u32 nrows = m - 64 * b < 64 ? m - 64 * b : 64;
				const bool row_on = R <= m;
				const u32 a = row_on ? adp[R - 1] : 0u;
				const bool keep_row = BANDED && b + 1 < n_bands && lane == 63;
				u32 cur = R << 16 | R, prev_up = 0;           // column 0: R adapter bases against gaps
				const i32 n_steps = W2 + (i32)nrows - 1;
				for (i32 t = 0; t < n_steps; ++t) {
					const i32 j = t - lane + 1;
					const u32 up_l = __shfl_up(cur, 1);
					u32 up = up_l, dg = prev_up;
					if (lane == 0 && j >= 1 && j <= W2) {
						if (b == 0) { up = (u32)j << 16 | (u32)j; dg = (u32)(j - 1) << 16 | (u32)(j - 1); }
						else { up = s_row[j]; dg = j == 1 ? ((R - 1) << 16 | (R - 1)) : s_row[j - 1]; }
					}
					if (row_on && j >= 1 && j <= W2) {
						const u32 c = a != w2[j - 1];
						const u32 Du = up >> 16, Dl = cur >> 16, Dd = dg >> 16;
						const u32 D = Dd + c < (Du < Dl ? Du : Dl) + 1 ? Dd + c : (Du < Dl ? Du : Dl) + 1;
						const u32 Lp = Du + 1 == D ? up : Dl + 1 == D ? cur : dg;     // edlib's traceback: up, else left, else diagonal
						cur = D << 16 | ((Lp & 0xffffu) + 1);
						if (keep_row) s_row[j] = cur;
					}
					prev_up = up_l;
				}
				if (BANDED) __syncthreads();
				if (b + 1 == n_bands) fin = cur;
			}
			L = (i32)((u32)__builtin_amdgcn_readlane((int)fin, last_lane) & 0xffffu);
		}
		if (lane == 0) {
			i32 *o = out + (u64)k * 4;
			o[0] = d; o[1] = s; o[2] = best_e; o[3] = L;
		}
	}
}
