// Test-only: longqc_amd/csrc/mapplan.hpp (the mapping stage's host decisions) behind a C ABI, compiled by tests/test_mapplan.py
// with g++ (LQ_EMU: lq_common.hpp without the HIP headers).  Every function takes one array of 64-bit words and fills one:
// shim_mapplan(name, in, n_in, out, out_cap, err, errlen) -> words written, or -1 with the exception's message in err.
// With -DMAPPLAN_SHIM_MAIN the file is a program: one case per line of stdin, "name word word ...", the output words per line of
// stdout ("! message" for an exception) -- the same cases once more, for a build with -fsanitize=address,undefined.
#define LQ_EMU 1
#include "../../longqc_amd/csrc/mapplan.hpp"
#include <cstdio>
#include <cstring>
#include <string>

namespace {
typedef std::vector<u64> Words;
Words slice(const u64 *&p, u64 n) { Words v(p, p + n); p += n; return v; }

// in: n_lanes, budget, g_begin, g_end, n, off[n], h_aq[n] -> batches, then q0 q1 of each
Words cut(const u64 *in)
{
	const int n_lanes = (int)in[0]; const u64 budget = in[1]; const u32 g_begin = (u32)in[2], g_end = (u32)in[3]; const u64 n = in[4];
	const u64 *p = in + 5;
	const Words off = slice(p, n), h_aq = slice(p, n);
	Words out{0};
	for (const auto &b : lq_cut_batches(off, h_aq, g_begin, g_end, budget, n_lanes)) { out.push_back(b.first); out.push_back(b.second); ++out[0]; }
	return out;
}

// in: budget, n_want, n, want[n_want], h_aq[n], h_qmoff[n] -> n_unique, want[n_unique], subsets, then per subset: ns, max_mini, sq[ns], sk[ns], so[ns + 1]
Words subsets(const u64 *in)
{
	const u64 budget = in[0], n_want = in[1], n = in[2];
	const u64 *p = in + 3;
	Words want = slice(p, n_want);
	const Words h_aq = slice(p, n), h_qmoff = slice(p, n);
	const std::vector<SecondPassSubset> subs = lq_second_pass_subsets(want, h_aq, h_qmoff, budget);
	Words out{want.size()};
	out.insert(out.end(), want.begin(), want.end());
	out.push_back(subs.size());
	for (const SecondPassSubset &S : subs) {
		out.push_back(S.sq.size()); out.push_back(S.max_mini);
		out.insert(out.end(), S.sq.begin(), S.sq.end()); out.insert(out.end(), S.sk.begin(), S.sk.end()); out.insert(out.end(), S.so.begin(), S.so.end());
	}
	return out;
}

// in: q_begin, q_stop, n_q, n_targets, seed_bucket, seed_segl, seed_chunk, with_segs, h_hq[n_q + 1], h_qmoff[n_q + 1]
// -> segments, bq entries, chunks, max_ne, max_nb, max_hits, sizeof(SeedQ), sizeof(SeedSeg), then per query mul nsl nseg seg0 cb bk,
//    has[n_q], bq_all, per chunk q_lo q_hi g_lo g_hi ne nb hits h0 big bq_at, and with_segs: per segment j0 j1 q ord
Words geometry(const u64 *in)
{
	const u32 n_q = (u32)in[2];
	const u64 *p = in + 8;
	const Words h_hq = slice(p, (u64)n_q + 1), h_qmoff = slice(p, (u64)n_q + 1);
	const SeedGeometry G = lq_seed_geometry(h_hq, h_qmoff, (u32)in[0], (u32)in[1], n_q, (u32)in[3], (u32)in[4], (u32)in[5], in[6]);
	Words out{G.segs.size(), G.bq_all.size(), G.chunks.size(), G.max_ne, G.max_nb, G.max_hits, sizeof(SeedQ), sizeof(SeedSeg)};
	for (const SeedQ &g : G.qg) for (u64 v : {(u64)g.mul, (u64)g.nsl, (u64)g.nseg, (u64)g.seg0, g.cb, g.bk}) out.push_back(v);
	out.insert(out.end(), G.has.begin(), G.has.end());
	out.insert(out.end(), G.bq_all.begin(), G.bq_all.end());
	for (const SeedChunk &c : G.chunks) for (u64 v : {(u64)c.q_lo, (u64)c.q_hi, (u64)c.g_lo, (u64)c.g_hi, c.ne, c.nb, c.hits, c.h0, (u64)c.big, (u64)c.bq_at}) out.push_back(v);
	if (in[7]) for (const SeedSeg &s : G.segs) for (u64 v : {s.j0, s.j1, (u64)s.q, (u64)s.ord}) out.push_back(v);
	return out;
}

// in: max_nm, max_tlen, max_qlen, n_targets, n_min, max_hits -> jb, db, rb, the filter can run
Words record_bits(const u64 *in)
{
	const SeedRecordBits b = lq_seed_record_bits(in[0], (u32)in[1], (u32)in[2], (u32)in[3]);
	return Words{b.jb, b.db, b.rb, lq_seed_filter_fits((u32)in[4], b, in[5]) ? 1u : 0u};
}
// in: n_min, jb, db, rb, max_hits -> the filter can run (a layout stated, not derived)
Words filter_fits(const u64 *in) { return Words{lq_seed_filter_fits((u32)in[0], SeedRecordBits{(u32)in[1], (u32)in[2], (u32)in[3]}, in[4]) ? 1u : 0u}; }
Words bits_for(const u64 *in) { return Words{lq_bits_for(in[0])}; }
// in: free, hbm_reserve, surv_cap, n_lanes
Words budget(const u64 *in) { return Words{lq_lane_anchor_budget(in[0], in[1], in[2], (int)in[3])}; }
Words clamp(const u64 *in) { return Words{lq_clamp_anchor_budget(in[0])}; }
// in: anchor_budget, nA_total
Words arena(const u64 *in) { return Words{(u64)lq_arena_need(in[0], in[1])}; }
// in: bucketed, q_begin, n_written, group_hits
Words few(const u64 *in) { return Words{lq_first_pass_leaves_few(in[0] != 0, (u32)in[1], in[2], in[3]) ? 1u : 0u}; }

const struct { const char *name; Words (*f)(const u64 *); } table[] = {
	{"cut", cut}, {"subsets", subsets}, {"geometry", geometry}, {"record_bits", record_bits}, {"filter_fits", filter_fits}, {"bits_for", bits_for},
	{"budget", budget}, {"clamp", clamp}, {"arena", arena}, {"few", few},
};
Words dispatch(const char *name, const u64 *in)
{
	for (const auto &e : table) if (!strcmp(e.name, name)) return e.f(in);
	throw std::invalid_argument("no such function");
}
}

extern "C" long long shim_mapplan(const char *name, const uint64_t *in, uint64_t n_in, uint64_t *out, uint64_t out_cap, char *err, size_t errlen)
{
	try {
		(void)n_in;
		const Words w = dispatch(name, in);
		if (w.size() > out_cap) throw std::length_error("the test's buffer is too small");
		std::copy(w.begin(), w.end(), out);
		return (long long)w.size();
	} catch (const std::exception &e) { if (err && errlen) snprintf(err, errlen, "%s", e.what()); return -1; }
}

#ifdef MAPPLAN_SHIM_MAIN
int main()
{
	std::string line;
	for (int ch; (ch = getchar()) != EOF; ) {
		if (ch != '\n') { line.push_back((char)ch); continue; }
		char name[32] = "";
		int at = 0;
		if (sscanf(line.c_str(), "%31s%n", name, &at) != 1) return 2;
		Words in;
		unsigned long long v; int used;
		for (const char *p = line.c_str() + at; sscanf(p, "%llu%n", &v, &used) == 1; p += used) in.push_back(v);
		in.push_back(0);                                        // (a case may have no input words: in.data() stays valid)
		try {
			for (u64 w : dispatch(name, in.data())) printf("%llu ", (unsigned long long)w);
			printf("\n");
		} catch (const std::exception &e) { printf("! %s\n", e.what()); }
		line.clear();
	}
	return 0;
}
#endif
