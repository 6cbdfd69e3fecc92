// longqc_amd/csrc/bamscan.hpp -- the host side of kernels_bamscan.hpp: one scan for BAM records over a range of inflated bytes on the
// device.  The result has FxScan's shape and lives in FxScan's tables -- rows, info, sseg, qseg on the device, h_rows, the counts and
// the resume position on the host -- so the reader's DeviceParse, names() and seg_start() serve both; n_lines counts the candidates
// examined.  Three waits per scan: the number of candidates, the number of records, the rows.
#pragma once
#include "fxscan.hpp"
#include "kernels_bamscan.hpp"

struct BamScan : FxScan {
	DBuf link;
	bool fetch_rows = true;                                   // false: h_rows stays empty, the rows are the device's alone (polread.cpp fetches them when it needs them)

	// d[0 .. n): the bytes (d + n + 16 readable); the parser stands at start_pos, a record boundary behind the BAM header.  Positions in
	// rows, segments and resume_pos are relative to d.  with_qual: the quality segments name the file's bytes, else LQ_GATHER_FILL.
	void run_bam(hipStream_t stream, const u8 *d, u64 n, u64 start_pos, bool with_qual)
	{
		n_rows = n_sseg = n_qseg = n_lines = bases = 0; h_rows.clear();
		resume_pos = start_pos; resume_last_char = 0;
		const u64 org = (u64)((uintptr_t)d & 15), lo64 = org + start_pos, hi64 = org + n;
		if (lo64 >= hi64 || hi64 >= LQ_FXSCAN_MAX_BYTES) return;
		const u8 *base = d - org;
		const u32 lo = (u32)lo64, hi = (u32)hi64;
		const u64 n_tiles = ((u64)hi - (lo & ~15u) + LQ_FXSCAN_TILE - 1) / LQ_FXSCAN_TILE;
		cols.ensure((size_t)n_tiles * 8); totals.ensure(16 * 8);
		u64 *tot = totals.as<u64>();
		LQ_LAUNCH(k_bam_candidates, grid(n_tiles), LQ_FXSCAN_THREADS, stream, base, lo, hi, n_tiles, cols.as<u64>(), 0, (u32*)nullptr);
		LQ_LAUNCH(k_fx_tilescan, 1, LQ_FXSCAN_THREADS, stream, cols.as<u64>(), n_tiles, 1u, tot);
		LQ_HIP_CHECK(hipGetLastError());
		u64 found = 0;
		LQ_HIP_CHECK(hipMemcpyAsync(&found, tot, 8, hipMemcpyDeviceToHost, stream));
		LQ_HIP_CHECK(hipStreamSynchronize(stream));
		n_lines = found + 1;                                      // (entry 0: the start)
		const u32 nc = (u32)n_lines;
		cand.ensure((size_t)nc * 4); link.ensure((size_t)nc * 16);
		jump0.ensure(((size_t)nc + 1) * 4); jump1.ensure(((size_t)nc + 1) * 4); mark.ensure(((size_t)nc + 1) * 4);
		LQ_LAUNCH(k_bam_candidates, grid(n_tiles), LQ_FXSCAN_THREADS, stream, base, lo, hi, n_tiles, cols.as<u64>(), 1, cand.as<u32>());
		const u64 l_tiles = ((u64)nc + 1 + LQ_FXSCAN_LINE_TILE - 1) / LQ_FXSCAN_LINE_TILE, e_tiles = ((u64)nc + LQ_FXSCAN_LINE_TILE - 1) / LQ_FXSCAN_LINE_TILE;
		LQ_LAUNCH(k_bam_link, grid(l_tiles), LQ_FXSCAN_THREADS, stream, base, hi, (const u32*)cand.as<u32>(), nc, link.as<uint4>(), jump0.as<u32>(), mark.as<u32>());
		u32 *jin = jump0.as<u32>(), *jout = jump1.as<u32>();
		for (u64 reach = 1; reach < n_lines; reach *= 2) {        // after a round the first 2 * reach records of the chain are marked
			LQ_LAUNCH(k_fx_jump, grid(l_tiles), LQ_FXSCAN_THREADS, stream, (const u32*)jin, jout, mark.as<u32>(), nc);
			std::swap(jin, jout);
		}
		ecols.ensure((size_t)e_tiles * LQ_BAMSCAN_EMIT_COLS * 8);
		const auto emit = [&](int phase) {
			LQ_LAUNCH(k_bam_emit, grid(e_tiles), LQ_FXSCAN_THREADS, stream, base, (u32)org, (const u32*)cand.as<u32>(), nc, (const uint4*)link.as<uint4>(), (const u32*)mark.as<u32>(),
			          ecols.as<u64>(), phase, with_qual ? 1 : 0, rows.as<FxRow>(), info.as<FxInfo>(), sseg.as<GatherSeg>(), qseg.as<GatherSeg>(), resume.as<u32>());
		};
		emit(0);
		LQ_LAUNCH(k_fx_tilescan, 1, LQ_FXSCAN_THREADS, stream, ecols.as<u64>(), e_tiles, (u32)LQ_BAMSCAN_EMIT_COLS, tot + 8);
		LQ_HIP_CHECK(hipGetLastError());
		u64 h_e[LQ_BAMSCAN_EMIT_COLS];
		LQ_HIP_CHECK(hipMemcpyAsync(h_e, tot + 8, sizeof(h_e), hipMemcpyDeviceToHost, stream));
		LQ_HIP_CHECK(hipStreamSynchronize(stream));
		if (!h_e[0]) return;
		n_rows = h_e[0]; n_sseg = n_qseg = h_e[1]; bases = h_e[2];
		rows.ensure((size_t)n_rows * sizeof(FxRow)); info.ensure((size_t)n_rows * sizeof(FxInfo)); resume.ensure(8);
		sseg.ensure((size_t)(n_sseg + 1) * sizeof(GatherSeg)); qseg.ensure((size_t)(n_qseg + 1) * sizeof(GatherSeg));
		emit(1);
		LQ_HIP_CHECK(hipGetLastError());
		u32 h_res = 0;
		if (fetch_rows) {
			h_rows.resize((size_t)n_rows);
			LQ_HIP_CHECK(hipMemcpyAsync(h_rows.data(), rows.p, (size_t)n_rows * sizeof(FxRow), hipMemcpyDeviceToHost, stream));
		}
		LQ_HIP_CHECK(hipMemcpyAsync(&h_res, resume.p, 4, hipMemcpyDeviceToHost, stream));
		LQ_HIP_CHECK(hipStreamSynchronize(stream));
		resume_pos = h_res;
	}
};
