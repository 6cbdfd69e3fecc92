// longqc_amd/csrc/mapplan.hpp -- what the host decides while a part is mapped, as plain functions: the batch cut, the second
// pass's subsets, the seed filter's geometry, the records' bit layout and the lanes' share of the HBM.  Host only: no HIP, no
// buffers, no handle -- engine.cpp's steps (map_part, map_batch, seed_filter, plan_part) size and launch from what these return,
// tests/test_mapplan.py calls them through tests/emu/mapplan_shim.cpp.
#pragma once
#include "seed_geom.hpp"
#include <algorithm>
#include <stdexcept>
#include <utility>
#include <vector>

// ---- the batch cut (map_part) ----
// As few batches as the work space allows, a multiple of the lane count, of about equal totals of `off` (the anchors the first
// pass writes, or the seed hits): every batch has a serial critical path that does not shrink with the batch.  (Cutting the
// last round finer was measured on MI355X at configs[2] in round 3: 1.75-1.78 s per step against 1.68-1.70 s; round 4: the
// queries in six chunks with the survivors of a chunk decided under the mapping of the chunk before: 1160 ms per step against 888;
// round 6: one batch per lane cut by the seed hits, each lane running the filter for its own batch -- see plan_part.)
// -> [q0, q1) of every batch: they tile [g_begin, g_end) in order; only a single query may exceed the budget.
inline std::vector<std::pair<u32, u32>> lq_cut_batches(const std::vector<u64> &off, const std::vector<u64> &h_aq, u32 g_begin, u32 g_end, u64 anchor_budget, int n_lanes)
{
	std::vector<std::pair<u32, u32>> batches;
	const u64 total = off[g_end] - off[g_begin];
	u64 nb = (total + anchor_budget - 1) / anchor_budget;
	if (nb < (u64)n_lanes && h_aq[g_end] - h_aq[g_begin] >= ((u64)n_lanes << 24)) nb = n_lanes;   // (by the seed hits, not by what the filter left of them: the second pass works on the hits)
	if (nb > (u64)n_lanes) nb = (nb + n_lanes - 1) / n_lanes * n_lanes;
	if (nb == 0) nb = 1;
	u64 left = nb;
	for (u32 q0 = g_begin; q0 < g_end; ) {
		const u64 rem = off[g_end] - off[q0];
		const u64 lim = std::min(anchor_budget, left > 1 ? (rem + left - 1) / left : rem);
		u32 q1 = q0 + 1;
		while (q1 < g_end && off[q1 + 1] - off[q0] <= lim) ++q1;
		batches.emplace_back(q0, q1);
		q0 = q1;
		if (left > 1) --left;
	}
	return batches;
}

// ---- the second pass's subsets (map_batch) ----
// want: the run keys the first pass listed, query << 32 | run; sorted and made unique in place (the device gets them so).  The
// queries that own one, in order, are cut into subsets of at most anchor_budget seed hits (a query above it goes alone):
// sq the queries, sk which of them go through klib's passes (more than LQ_RS_MIN anchors), so their anchor offsets.
// max_mini sizes the grid of the subset's k_seed_emit: the most minimizers of a query of this subset *or of an earlier one of
// the batch* -- a running maximum, not reset per subset (blocks beyond a query's minimizers find nothing to do).
struct SecondPassSubset { std::vector<u32> sq, sk; std::vector<u64> so; u64 max_mini; };
inline std::vector<SecondPassSubset> lq_second_pass_subsets(std::vector<u64> &want, const std::vector<u64> &h_aq, const std::vector<u64> &h_qmoff, u64 anchor_budget)
{
	std::sort(want.begin(), want.end());
	want.erase(std::unique(want.begin(), want.end()), want.end());
	std::vector<u32> fq;
	for (u64 k : want) if (fq.empty() || fq.back() != (u32)(k >> 32)) fq.push_back((u32)(k >> 32));
	std::vector<SecondPassSubset> subsets;
	u64 max_mini = 0;
	for (size_t i = 0; i < fq.size(); ) {
		SecondPassSubset S; S.so.push_back(0);
		size_t k = i;
		while (k < fq.size() && (k == i || S.so.back() + (h_aq[fq[k] + 1] - h_aq[fq[k]]) <= anchor_budget)) {
			const u64 len = h_aq[fq[k] + 1] - h_aq[fq[k]];
			S.sq.push_back(fq[k]); S.sk.push_back(len > LQ_RS_MIN ? 1u : 0u); S.so.push_back(S.so.back() + len);
			max_mini = std::max<u64>(max_mini, h_qmoff[fq[k] + 1] - h_qmoff[fq[k]]);
			++k;
		}
		S.max_mini = max_mini;
		subsets.push_back(std::move(S));
		i = k;
	}
	return subsets;
}

// ---- the seed filter's geometry (seed_filter) ----
// From the hits before every query (h_hq) and its minimizers (h_qmoff): per query with hits its slices of targets (about
// seed_bucket hits each, at most LQ_SD_SL_BIG and half the targets) and its segments of seed_segl minimizers; the queries
// [q_begin, q_stop) in chunks of at most max(seed_chunk, the largest query) hits.  cb / bk are a query's first piece and first
// bucket in its chunk; bq_all holds, chunk after chunk, every query's bk and then the chunk's bucket count.
struct SeedChunk { u32 q_lo, q_hi, g_lo, g_hi; u64 ne, nb, hits, h0; bool big; size_t bq_at; };   // queries, segments; pieces, buckets, hits; big: a query with more than LQ_SD_SL_SMALL slices
struct SeedGeometry { std::vector<SeedQ> qg; std::vector<SeedSeg> segs; std::vector<u32> has, bq_all; std::vector<SeedChunk> chunks; u64 max_ne = 0, max_nb = 0, max_hits = 0; };   // has: the query has hits; max_*: over the chunks
inline SeedGeometry lq_seed_geometry(const std::vector<u64> &h_hq, const std::vector<u64> &h_qmoff, u32 q_begin, u32 q_stop, u32 n_q, u32 n_targets,
                                     u32 seed_bucket, u32 seed_segl, u64 seed_chunk)
{
	SeedGeometry G;
	n_targets = std::max<u32>(n_targets, 1);
	G.qg.assign(n_q, SeedQ{0, 0, 0, 0, 0, 0});                // (the queries outside [q_begin, q_stop) stay zero)
	G.has.assign(n_q, 0);
	u64 max_hq = 0;
	for (u32 i = 0; i < n_q; ++i) max_hq = std::max(max_hq, h_hq[i + 1] - h_hq[i]);
	if (max_hq >= 0xfffffff0ULL) throw std::domain_error("more than 2^32 seed hits of one query against one index part");
	const u64 chunk_cap = std::max<u64>(seed_chunk, max_hq);
	q_stop = std::min(q_stop, n_q);
	u64 n_segs = 0;                                           // (the segments are written once their number is known to be in range)
	for (u32 i = q_begin; i < q_stop; ) {
		SeedChunk c; c.q_lo = i; c.g_lo = (u32)n_segs; c.ne = 0; c.nb = 0; c.hits = 0; c.h0 = h_hq[i]; c.big = false; c.bq_at = G.bq_all.size();
		while (i < q_stop && (c.hits == 0 || c.hits + (h_hq[i + 1] - h_hq[i]) <= chunk_cap)) {
			const u64 hq = h_hq[i + 1] - h_hq[i], nm = h_qmoff[i + 1] - h_qmoff[i];
			SeedQ g{0, 0, 0, (u32)n_segs, c.ne, c.nb};
			if (hq) {
				G.has[i] = 1;
				u64 nsl = (hq + seed_bucket - 1) / seed_bucket;
				nsl = std::min<u64>(nsl, std::min<u64>(LQ_SD_SL_BIG, std::max<u32>(n_targets / 2, 1)));
				g.nsl = (u32)std::max<u64>(nsl, 1);
				g.mul = g.nsl == 1 ? 0u : (u32)((((u64)g.nsl) << 32) / n_targets);       // slice of rid = rid * mul >> 32 < nsl for every rid < n_targets
				g.nseg = (u32)((nm + seed_segl - 1) / seed_segl);
				n_segs += g.nseg;
				if (g.nsl > LQ_SD_SL_SMALL) c.big = true;
				c.ne += (u64)g.nsl * g.nseg; c.nb += g.nsl; c.hits += hq;
			}
			G.bq_all.push_back((u32)g.bk);
			G.qg[i] = g;
			++i;
		}
		G.bq_all.push_back((u32)c.nb);
		c.q_hi = i; c.g_hi = (u32)n_segs;
		if (c.ne >= 0xfffffff0ULL || c.nb >= 0x7ffffff0ULL) throw std::domain_error("seed filter: too many (query, slice, segment) pieces in one chunk");
		G.chunks.push_back(c);
	}
	if (n_segs >= 0x7ffffff0ULL) throw std::domain_error("seed filter: too many segments");
	G.segs.assign(n_segs, SeedSeg{0, 0, 0, 0, 0, 0});
	for (u32 i = q_begin; i < q_stop; ++i)
		for (u32 p = 0; p < G.qg[i].nseg; ++p) {
			SeedSeg &sg = G.segs[G.qg[i].seg0 + p];
			sg.j0 = h_qmoff[i] + (u64)p * seed_segl; sg.j1 = std::min<u64>(sg.j0 + seed_segl, h_qmoff[i + 1]); sg.q = i; sg.ord = p;
		}
	for (const SeedChunk &c : G.chunks) { G.max_ne = std::max(G.max_ne, c.ne); G.max_nb = std::max(G.max_nb, c.nb); G.max_hits = std::max(G.max_hits, c.hits); }
	return G;
}

// ---- the survivors' records (plan_part; SeedBits, kernels_seed.hpp) ----
// record = rid:rb | relative strand:1 | diagonal:db | minimizer inside its query:jb
inline u32 lq_bits_for(u64 v) { u32 b = 1; while (b < 63 && (v >> b)) ++b; return b; }   // bits that hold 0 .. v
struct SeedRecordBits { u32 jb, db, rb; };
inline SeedRecordBits lq_seed_record_bits(u64 max_nm, u32 max_tlen, u32 max_qlen, u32 n_targets) { return SeedRecordBits{lq_bits_for(max_nm - 1), lq_bits_for((u64)max_tlen + max_qlen + 257), lq_bits_for(n_targets ? n_targets - 1 : 0)}; }
// the filter can run: a run needs 2 .. 15 anchors (the pair counters), a record fits 64 bits with fields the kernels can shift by,
// and no query has more hits than a bucket's 31-bit offsets hold (max_hits: the most seed hits of one query)
inline bool lq_seed_filter_fits(u32 n_min, SeedRecordBits b, u64 max_hits)
{
	return n_min >= 2 && n_min <= 15 && b.jb + b.db + 1 + b.rb <= 64 && b.db <= 31 && b.jb <= 31 && max_hits < 0x7fff0000ULL;
}

// ---- the lanes' share of the HBM (map_part) ----
// The first part stands (reads, minimizers, index, the build's work space -- all kept for the parts to come, of which the
// first is the largest: index.c:244) and so do the queries: the lanes share a fraction of what is free now.  Per anchor a lane
// holds A and B (32 B), one record array (8), 20 B of scratch, digit + destination (5), ~12 B of lists and per-sub-array
// rows, ~6 B of runs and intervals, and the buffers grow with an eighth of head room: ~95 B, counted as
#define LQ_LANE_ANCHOR_BYTES 104
// (0.75 since round 4 -- it was 0.85: a lane's buffers now grow in more steps -- a small first pass, second passes of varying size -- and a
// block the stream-ordered pool got back is not always the one the next, larger request can use; at 0.85 the ultra-long
// slice of configs[4] ran the device out of memory inside the runtime (HSA_STATUS_ERROR_OUT_OF_RESOURCES))
#define LQ_LANE_HBM_SHARE 0.75
inline u64 lq_clamp_anchor_budget(u64 b) { return std::min<u64>(std::max<u64>(b, 1024), (1ULL << 31) - 4096); }   // (a record names its anchor in 31 bits)
// free: bytes free now; hbm_reserve: what the caller wants left (lqcov_reserve_hbm: e.g. the part it builds while this one is
// mapped) -- and then the survivors of that part's seed plan too: as many as this part's (surv_cap bytes), with the head room
// they grow by
inline u64 lq_lane_anchor_budget(u64 free, u64 hbm_reserve, u64 surv_cap, int n_lanes)
{
	u64 fr = free > hbm_reserve ? free - hbm_reserve : 0;
	const u64 sv = hbm_reserve ? surv_cap + surv_cap / 2 : 0;
	fr = fr > sv ? fr - sv : 0;
	return lq_clamp_anchor_budget((u64)((double)fr * LQ_LANE_HBM_SHARE / (double)LQ_LANE_ANCHOR_BYTES / n_lanes));
}
// a lane's arena: as much as its largest batch of this part can need
inline size_t lq_arena_need(u64 anchor_budget, u64 nA_total)
{
	size_t need = (size_t)std::min<u64>(anchor_budget, std::max<u64>(nA_total, 1)) * LQ_LANE_ANCHOR_BYTES / 9 * 8 + ((size_t)16 << 20);
#ifdef LQ_EMU
	need = std::min<size_t>(need, (size_t)64 << 20);            // (the test emulator fills fresh memory with a pattern)
#endif
	return need;
}
// The lanes work from arenas only where the first pass leaves a small part of the hits: a batch whose first pass fills the
// lane's share by itself -- ultra-long reads keep a third of their hits -- needs its buffers again in the second pass, and
// pieces of an arena are not given back: there the lanes allocate buffer by buffer, grow-only.
// bucketed: the plan holds survivors; q_begin: of the group that starts there; group_hits: the group's seed hits
inline bool lq_first_pass_leaves_few(bool bucketed, u32 q_begin, u64 n_written, u64 group_hits)
{
	return bucketed && q_begin == 0 && n_written * 4 <= group_hits;
}
