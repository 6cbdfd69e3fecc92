// longqc_amd/csrc/fxscan.hpp -- the host side of kernels_fxscan.hpp: one record scan over a range of bytes on the device.  The tables
// stay on the device (sseg, qseg, info: what the reader rebases into a chunk's lists); the rows, the counts and the resume state
// come back.  Three waits per scan: the number of lines, the number of records, the rows.  names(): the names of rows, gathered on
// the device (k_fx_names), for a host that does not hold the bytes; two waits, the blob's length and the blob.
#pragma once
#include "kernels_fxscan.hpp"
#include <vector>

struct FxScan {
	DBuf cols, totals, L4, L2, cand, jump0, jump1, mark, ecols, rows, info, sseg, qseg, resume;
	u64 n_rows = 0, n_sseg = 0, n_qseg = 0, n_lines = 0, bases = 0;
	u64 resume_pos = 0; int resume_last_char = 0;
	std::vector<FxRow> h_rows;

	static u32 grid(u64 n_tiles) { return (u32)std::min<u64>(std::max<u64>(n_tiles, 1), LQ_FXSCAN_MAX_BLOCKS); }

	// d[0 .. n): the bytes (d + n + 16 readable); the parser stands at start_pos with last_char, a clean start (reader.cpp).  Positions
	// in rows, segments and the resume state are relative to d.
	void run(hipStream_t stream, const u8 *d, u64 n, u64 start_pos, int last_char)
	{
		n_rows = n_sseg = n_qseg = n_lines = bases = 0; h_rows.clear();
		resume_pos = start_pos; resume_last_char = last_char;
		const u64 org = (u64)((uintptr_t)d & 15), lo64 = org + start_pos, hi64 = org + n;
		if (lo64 >= hi64 || hi64 >= LQ_FXSCAN_MAX_BYTES) return;
		const u8 *base = d - org;
		const u32 lo = (u32)lo64, hi = (u32)hi64;
		const u64 n_tiles = ((u64)hi - (lo & ~15u) + LQ_FXSCAN_TILE - 1) / LQ_FXSCAN_TILE;
		cols.ensure((size_t)n_tiles * LQ_FXSCAN_LINE_COLS * 8); totals.ensure(16 * 8);
		u64 *tot = totals.as<u64>();
		LQ_LAUNCH(k_fx_lines, grid(n_tiles), LQ_FXSCAN_THREADS, stream, base, lo, hi, n_tiles, cols.as<u64>(), (const u64*)tot, 0, (uint4*)nullptr, (uint2*)nullptr);
		LQ_LAUNCH(k_fx_tilescan, 1, LQ_FXSCAN_THREADS, stream, cols.as<u64>(), n_tiles, (u32)LQ_FXSCAN_LINE_COLS, tot);
		LQ_HIP_CHECK(hipGetLastError());
		u64 h_tot[LQ_FXSCAN_LINE_COLS];
		LQ_HIP_CHECK(hipMemcpyAsync(h_tot, tot, sizeof(h_tot), hipMemcpyDeviceToHost, stream));
		LQ_HIP_CHECK(hipStreamSynchronize(stream));
		n_lines = h_tot[0] + 1;
		const u32 nl = (u32)n_lines;
		L4.ensure(((size_t)nl + 1) * 16); L2.ensure(((size_t)nl + 1) * 8); cand.ensure((size_t)nl * 16);
		jump0.ensure(((size_t)nl + 1) * 4); jump1.ensure(((size_t)nl + 1) * 4); mark.ensure(((size_t)nl + 1) * 4);
		LQ_LAUNCH(k_fx_lines, grid(n_tiles), LQ_FXSCAN_THREADS, stream, base, lo, hi, n_tiles, cols.as<u64>(), (const u64*)tot, 1, L4.as<uint4>(), L2.as<uint2>());
		const u64 l_tiles = ((u64)nl + 1 + LQ_FXSCAN_LINE_TILE - 1) / LQ_FXSCAN_LINE_TILE, e_tiles = ((u64)nl + LQ_FXSCAN_LINE_TILE - 1) / LQ_FXSCAN_LINE_TILE;
		LQ_LAUNCH(k_fx_candidates, grid(l_tiles), LQ_FXSCAN_THREADS, stream, base, (const uint4*)L4.as<uint4>(), (const uint2*)L2.as<uint2>(), nl, (u32)last_char, cand.as<uint4>(), jump0.as<u32>(), mark.as<u32>());
		u32 *jin = jump0.as<u32>(), *jout = jump1.as<u32>();
		for (u64 reach = 1; reach < n_lines; reach *= 2) {        // after a round the first 2 * reach candidates of the chain are marked
			LQ_LAUNCH(k_fx_jump, grid(l_tiles), LQ_FXSCAN_THREADS, stream, (const u32*)jin, jout, mark.as<u32>(), nl);
			std::swap(jin, jout);
		}
		ecols.ensure((size_t)e_tiles * LQ_FXSCAN_EMIT_COLS * 8);
		const auto emit = [&](int phase) {
			LQ_LAUNCH(k_fx_emit, grid(e_tiles), LQ_FXSCAN_THREADS, stream, base, (u32)org, (const uint4*)L4.as<uint4>(), (const uint2*)L2.as<uint2>(), nl, (u32)last_char, (const uint4*)cand.as<uint4>(),
			          (const u32*)mark.as<u32>(), ecols.as<u64>(), phase, rows.as<FxRow>(), info.as<FxInfo>(), sseg.as<GatherSeg>(), qseg.as<GatherSeg>(), resume.as<u32>());
		};
		emit(0);
		LQ_LAUNCH(k_fx_tilescan, 1, LQ_FXSCAN_THREADS, stream, ecols.as<u64>(), e_tiles, (u32)LQ_FXSCAN_EMIT_COLS, tot + 8);
		LQ_HIP_CHECK(hipGetLastError());
		u64 h_e[LQ_FXSCAN_EMIT_COLS];
		LQ_HIP_CHECK(hipMemcpyAsync(h_e, tot + 8, sizeof(h_e), hipMemcpyDeviceToHost, stream));
		LQ_HIP_CHECK(hipStreamSynchronize(stream));
		if (!h_e[0]) return;
		n_rows = h_e[0]; n_sseg = h_e[1]; n_qseg = h_e[2]; bases = h_e[3];
		rows.ensure((size_t)n_rows * sizeof(FxRow)); info.ensure((size_t)n_rows * sizeof(FxInfo)); resume.ensure(8);
		sseg.ensure((size_t)(n_sseg + 1) * sizeof(GatherSeg)); qseg.ensure((size_t)(n_qseg + 1) * sizeof(GatherSeg));
		emit(1); emit(2);
		LQ_HIP_CHECK(hipGetLastError());
		h_rows.resize((size_t)n_rows);
		u32 h_res[2] = {0, 0};
		LQ_HIP_CHECK(hipMemcpyAsync(h_rows.data(), rows.p, (size_t)n_rows * sizeof(FxRow), hipMemcpyDeviceToHost, stream));
		LQ_HIP_CHECK(hipMemcpyAsync(h_res, resume.p, 8, hipMemcpyDeviceToHost, stream));
		LQ_HIP_CHECK(hipStreamSynchronize(stream));
		resume_pos = h_res[0]; resume_last_char = (int)h_res[1];
	}

	// the names of d_rows[0 .. n) (rows on the device; positions count from d): h_names = every name and a NUL, h_name_off its n + 1
	// offsets, first_bad the first row whose name holds a byte of 0x80 or more (n: none)
	DBuf ncols, d_names, d_name_off;
	std::vector<char> h_names; std::vector<u64> h_name_off; u64 first_bad = 0;
	void names(hipStream_t stream, const u8 *d, const FxRow *d_rows, u64 n)
	{
		h_names.clear(); h_name_off.assign((size_t)n + 1, 0); first_bad = n;
		if (!n) return;
		const u64 n_tiles = (n + LQ_FXSCAN_LINE_TILE - 1) / LQ_FXSCAN_LINE_TILE;
		ncols.ensure((size_t)n_tiles * 8); totals.ensure(16 * 8); d_name_off.ensure((size_t)(n + 1) * 8);
		u64 *tot = totals.as<u64>();
		LQ_LAUNCH(k_fx_names, grid(n_tiles), LQ_FXSCAN_THREADS, stream, d, d_rows, n, ncols.as<u64>(), 0, (char*)nullptr, (u64*)nullptr, (unsigned long long*)(tot + 13));
		LQ_LAUNCH(k_fx_tilescan, 1, LQ_FXSCAN_THREADS, stream, ncols.as<u64>(), n_tiles, 1u, tot + 12);
		LQ_HIP_CHECK(hipGetLastError());
		u64 bytes = 0;
		LQ_HIP_CHECK(hipMemcpyAsync(&bytes, tot + 12, 8, hipMemcpyDeviceToHost, stream));
		LQ_HIP_CHECK(hipStreamSynchronize(stream));
		d_names.ensure((size_t)bytes);
		LQ_LAUNCH(k_fx_names, grid(n_tiles), LQ_FXSCAN_THREADS, stream, d, d_rows, n, ncols.as<u64>(), 1, d_names.as<char>(), d_name_off.as<u64>(), (unsigned long long*)(tot + 13));
		LQ_HIP_CHECK(hipGetLastError());
		h_names.resize((size_t)bytes);
		LQ_HIP_CHECK(hipMemcpyAsync(h_names.data(), d_names.p, (size_t)bytes, hipMemcpyDeviceToHost, stream));
		LQ_HIP_CHECK(hipMemcpyAsync(h_name_off.data(), d_name_off.p, (size_t)(n + 1) * 8, hipMemcpyDeviceToHost, stream));
		LQ_HIP_CHECK(hipMemcpyAsync(&first_bad, tot + 13, 8, hipMemcpyDeviceToHost, stream));
		LQ_HIP_CHECK(hipStreamSynchronize(stream));
	}

	// where record r's segments start in sseg / qseg (r == n_rows: their ends)
	void seg_start(hipStream_t stream, u64 r, u64 *s, u64 *q)
	{
		if (r >= n_rows) { *s = n_sseg; *q = n_qseg; return; }
		FxInfo f;
		LQ_HIP_CHECK(hipMemcpyAsync(&f, info.as<FxInfo>() + r, sizeof(f), hipMemcpyDeviceToHost, stream));
		LQ_HIP_CHECK(hipStreamSynchronize(stream));
		*s = f.sseg; *q = f.qseg;
	}
};
