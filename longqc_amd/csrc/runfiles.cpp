// longqc_amd/csrc/runfiles.cpp -- the whole run from files (minimap2-coverage.c:406-617): lqcov_handle::run_files and the table as
// text.  Host code only: what runs on the device is behind the handle's calls (engine.cpp), the index file's bytes are mmi.hpp's.
#include "engine.hpp"
#include "fastx.hpp"
#include "fastx_mem.hpp"
#include "mmi.hpp"
#include <cstdio>
#include <cstring>
#include <cmath>
#include <cinttypes>
#include <algorithm>
#include <future>
#include <functional>

// ---- the table ----------------------------------------------------------------------------------------
// rows as text (minimap2-coverage.c:567-605); name_of(i) = the name of the query of row i
void lq_format_rows(FILE *out, int filter_flag, const lqcov_row *rows, u32 n_rows, const lqcov_region *regs, const lqcov_region *mregs,
                    const std::function<const char *(u32)> &name_of)
{
	std::string line;
	char buf[128];
	for (u32 i = 0; i < n_rows; ++i) {
		const lqcov_row &r = rows[i];
		const double div = r.n_match > 0 ? logf((float)r.n_mini / (float)(int32_t)r.n_match) / r.avg_k : 1.0;   // :563
		double mq;
		if (r.has_qual) mq = -10 * log10(r.qual_psum / (int)r.qlen);                                          // lqutils.c:57
		else { volatile double z = 0.0; volatile int zl = 0; mq = -10 * log10(z / zl); }                                      // FASTA query: the reference's 0/0
		line.clear();
		line += name_of(i); line += '\t';
		snprintf(buf, sizeof(buf), "%d\t%" PRIu64 "\t", (int)r.qlen, r.lambda); line += buf;
		if (r.n_reg > 0) {
			u32 tot = 0;
			for (u32 k = 0; k < r.n_reg; ++k) {
				const lqcov_region &g = regs[r.reg_off + k];
				snprintf(buf, sizeof(buf), "%s%d-%d", k ? "," : "", (int)g.start, (int)g.end); line += buf;
				tot += g.end - g.start;
			}
			line += '\t';
			if (r.n_mreg > 0) {
				for (u32 k = 0; k < r.n_mreg; ++k) {
					const lqcov_region &g = mregs[r.mreg_off + k];
					snprintf(buf, sizeof(buf), "%s%d-%d", k ? "," : "", (int)g.start, (int)g.end); line += buf;
				}
			} else line += '0';
			if (filter_flag) snprintf(buf, sizeof(buf), "\t%.3f\t%.3f\t%.3f\t0.0\n", (double)tot / (int)r.qlen, mq, div);
			else snprintf(buf, sizeof(buf), "\t%.3f\t%.3f\t%.3f\t%.3f\n", (double)r.lambda / tot, mq, div, (double)r.lambda2 / tot);
			line += buf;
		} else {
			snprintf(buf, sizeof(buf), "0\t0\t0.0\t%.3f\t%.3f\t0.0\n", mq, div); line += buf;
		}
		fwrite(line.data(), 1, line.size(), out);
	}
}

void lqcov_handle::write_table(FILE *out)
{
	if (!finished) throw std::logic_error("finish() has not run");
	lq_format_rows(out, P.filter_flag, rows.data(), q.n, regs.data(), mregs.data(), [&](u32 i) { return q.names[q_inv[i]].c_str(); });
}

void lqcov_handle::write_table_set(u32 set, FILE *out)
{
	if (!finished) throw std::logic_error("finish() has not run");
	if (set + 1 >= set_first.size()) throw std::invalid_argument("no such query set");
	const u32 a = set_first[set];
	lq_format_rows(out, P.filter_flag, rows.data() + a, set_first[set + 1] - a, regs.data(), mregs.data(), [&](u32 i) { return q.names[q_inv[a + i]].c_str(); });
}

namespace {

struct Closer { FILE *f; ~Closer() { if (f) fclose(f); } };

// ---- the target: sequences, or an index file? (mm_idx_is_idx, index.c:481-498) --------------------------
struct TargetProbe { bool is_idx = false; MmiHeader hdr{}; };

TargetProbe probe_target(const char *target)
{
	FILE *t = fopen(target, "rb");
	if (!t) throw lq_open_error(target);
	Closer closer{t};
	TargetProbe p;
	p.is_idx = mmi_read_header(t, p.hdr);
	return p;
}

// ---- the queries (read, upload, sketch: minimap2-coverage.c:406-431) -------------------------------------
void read_all(const char *path, ReadBatch &b)
{
	FastxReader fq(path);
	while (fq.read_minibatch(INT64_MAX, b, true) > 0) {}
}

void append_batch(ReadBatch &qb, const ReadBatch &b)
{
	const u64 sb = qb.seq.size(), nb = qb.names.size();
	qb.seq.insert(qb.seq.end(), b.seq.begin(), b.seq.end()); qb.qual.insert(qb.qual.end(), b.qual.begin(), b.qual.end());
	qb.names.insert(qb.names.end(), b.names.begin(), b.names.end());
	for (u32 i = 1; i < b.seq_off.size(); ++i) qb.seq_off.push_back(sb + b.seq_off[i]);
	for (u32 i = 1; i < b.name_off.size(); ++i) qb.name_off.push_back(nb + b.name_off[i]);
	qb.any_qual = qb.any_qual || b.any_qual;
}

void load_query_file(lqcov_handle &h, const char *query, FILE *log, double t_run0)
{
	ReadBatch qb;
	read_all(query, qb);
	const double tq = lq_now_s();
	h.set_queries(qb.size(), qb.seq.data(), qb.seq_off.data(), qb.any_qual ? qb.qual.data() : nullptr, qb.names.data(), qb.name_off.data());
	if (log) fprintf(log, "[lqcov] loaded %u query sequence(s), %" PRIu64 " bases, %" PRIu64 " minimizers (read %.3f s, upload + sketch %.3f s)\n", qb.size(), qb.bases(), h.q.n_mini, tq - t_run0, lq_now_s() - tq);
}

// the files one after the other, each parsed as a call of its own parses it
void load_query_sets(lqcov_handle &h, const lqcov_handle::QuerySetFiles &sets, FILE *log, double t_run0)
{
	ReadBatch qb;
	std::vector<u32> first{0};
	int with_qual = -1;
	for (size_t f = 0; f < sets.paths.size(); ++f) {
		ReadBatch b;
		read_all(sets.paths[f], b);
		if (b.size()) {
			if (with_qual >= 0 && with_qual != (int)b.any_qual)
				throw std::domain_error("query sets with qualities mixed with sets without: the mean quality column is per call (FASTQ and FASTA sets cannot share one)");
			with_qual = (int)b.any_qual;
		}
		append_batch(qb, b);
		first.push_back(qb.size());
	}
	const double tq = lq_now_s();
	h.set_query_sets(qb.size(), qb.seq.data(), qb.seq_off.data(), qb.any_qual ? qb.qual.data() : nullptr, qb.names.data(), qb.name_off.data(),
	                 (u32)sets.paths.size(), first.data(), sets.med.data(), sets.good.data());
	if (log) fprintf(log, "[lqcov] loaded %u query sequence(s) in %zu set(s), %" PRIu64 " bases, %" PRIu64 " minimizers (read %.3f s, upload + sketch %.3f s)\n", qb.size(), sets.paths.size(), qb.bases(), h.q.n_mini, tq - t_run0, lq_now_s() - tq);
}

void load_queries(lqcov_handle &h, const char *query, const lqcov_handle::QuerySetFiles *sets, FILE *log, double t_run0)
{
	LQ_HIP_CHECK(hipSetDevice(h.device));                         // (may run on a thread of its own)
	if (sets) load_query_sets(h, *sets, log, t_run0);
	else load_query_file(h, query, log, t_run0);
}

// The queries while the host makes the first part -- parse, page-locked buffers, 2-bit packing, all host work; joined before
// anything of the targets touches the device (run_target_parts).  A prebuilt index has no such host work: loaded here and now.
std::future<void> start_queries(lqcov_handle &h, const char *query, const lqcov_handle::QuerySetFiles *sets, FILE *log, double t_run0, bool on_a_thread)
{
#ifndef LQ_EMU
	if (on_a_thread) return std::async(std::launch::async, load_queries, std::ref(h), query, sets, log, t_run0);
#endif
	load_queries(h, query, sets, log, t_run0);                    // (the test emulator runs its kernels on the calling thread, one at a time)
	return std::future<void>();
}

struct QueriesJoin { std::future<void> &f; ~QueriesJoin() { if (f.valid()) { try { f.get(); } catch (...) {} } } };   // (never leave the task behind when something else throws)

void map_part_logged(lqcov_handle &h, Part &pt, int n_parts, FILE *log)
{
	const double tm0 = lq_now_s();
	h.map_part(pt);
	if (log) fprintf(log, "[lqcov] part %d: mapped %u queries in %.3f s, %" PRIu64 " anchors (%" PRIu64 " written; so far %" PRIu64 " runs of %" PRIu64 " queries chained in klib's order, %" PRIu64 " anchors)\n",
	                 n_parts, h.q.n, lq_now_s() - tm0, h.last_n_anchors, h.last_n_written, (u64)h.stat_sens_runs, (u64)h.stat_p2_queries, (u64)h.stat_p2_anchors);
}

// ---- a prebuilt index as the target: its parts one after the other (mm_idx_reader_read, index.c:500-540) ----
void run_prebuilt_parts(lqcov_handle &h, const char *target, const MmiHeader &ih, bool has_query, FILE *log)
{
	const i32 ihpc = (i32)(ih.flag & 1);
	if (ih.k != h.P.k || ih.w != h.P.w || (ihpc != 0) != (h.P.hpc != 0)) {
		if (log) fprintf(log, "[WARNING] Indexing parameters (-k, -w or -H) overridden by parameters used in the prebuilt index.\n");
		h.adopt_index_params(ih.k, ih.w, ihpc);
	}
	FILE *fi = fopen(target, "rb");
	if (!fi) throw lq_open_error(target);
	Closer fi_closer{fi};
	for (int n_parts = 0;; ++n_parts) {
		h.parts.emplace_back(new Part());
		const int id = (int)h.parts.size() - 1;
		h.parts[id]->live = true;
		if (!h.load_part(fi, *h.parts[id])) { h.parts[id].reset(); break; }
		Part &pt = *h.parts[id];
		if (log) fprintf(log, "[lqcov] part %d (prebuilt): %u target sequence(s), %" PRIu64 " minimizers, %" PRIu64 " distinct, mid_occ = %d\n",
		                 n_parts, pt.rs.n, pt.rs.n_mini, pt.n_keys, h.mid_occ);
		if (has_query) h.map_part(pt);
		h.parts[id].reset();
	}
}

// ---- sequences as the target: the host side ---------------------------------------------------------------
// One part as the host hands it to the build: the streaming reader's mini-batches, or 2-bit packed in page-locked memory.
struct HostPart {
	bool packed = false, last = false;                         // last: the input ended inside this part
	std::vector<ReadBatch> bs;                                 // streaming form (ASCII)
	u64 *codes = nullptr; u32 *amb = nullptr; u64 cap_words = 0;   // packed form, page-locked
	std::vector<u32> lens; std::vector<char> names; std::vector<u64> name_off{0};
	u32 n = 0; u64 bases = 0;
	std::atomic<bool> any_amb{false};                           // packed form: a read of the part holds an ambiguous base
	bool empty() const { return packed ? n == 0 : bs.empty(); }
	~HostPart() { if (codes) hipHostFree(codes); if (amb) hipHostFree(amb); }
};

struct FlatRec { const u8 *name; u32 name_len; const u8 *seq; u32 seq_len; };

// The target file and the parts made from it.  A plain file: parsed by many threads from the mapping and 2-bit packed into
// page-locked memory (fastx_mem.hpp); gzip or a pipe: the streaming reader, one thread like the reference's kseq.  Two slots:
// one part is uploaded while the next one is made.
struct TargetHost {
	lqcov_handle &h;
	const int64_t chunk;                                       // bases of a mini-batch (index.c:316)
	HostPart hp[2];
	MemFastx mf;
	MemRecords recs;
	std::vector<FlatRec> flat;
	std::vector<std::pair<size_t, size_t>> ranges;             // records of every part (memory path)
	size_t next_range = 0;
	std::unique_ptr<FastxReader> ft;
	bool mem = false;
	double t_host[2] = {0, 0}, t_alloc[2] = {0, 0};

	TargetHost(lqcov_handle &h_, int64_t chunk_) : h(h_), chunk(chunk_) {}
	void open(const char *target, FILE *log);
	void produce(int slot);
	void produce_streamed(HostPart &p);
	void produce_packed(HostPart &p, double &t_alloc_slot);
	void pack_reads(HostPart &p, size_t r0, const std::vector<u64> &coff);
};

void TargetHost::open(const char *target, FILE *log)
{
	const Knobs &K = h.K;
	mem = K.parse_threads != 1 && mf.open(target);
	const double t_parse0 = lq_now_s();
	if (mem) {
		// (records of several lines are copied out of the mapping: a wrapped FASTA of many gigabases would be held twice, so
		// past LQCOV_PARSE_SIDE bytes of copies the file is streamed like a gzip instead, one part in memory at a time)
		lq_parse_all(mf, K.parse_threads, K.parse_piece, recs, K.parse_side);
		if (recs.too_wrapped) { mem = false; mf.close(); if (log) fprintf(log, "[lqcov] target records span several lines: streaming reader\n"); }
	}
	if (!mem) { ft.reset(new FastxReader(target)); return; }
	flat.reserve(recs.n_recs);
	for (MemPiece &pc : recs.pieces) for (MemRec &r : pc.recs)
		flat.push_back(FlatRec{mf.data() + r.name_off, r.name_len, (r.own ? pc.side.data() : mf.data()) + r.seq_off, r.seq_len});
	for (const auto &rg : lq_part_ranges(flat.size(), [&](size_t i) { return (u64)flat[i].seq_len; }, h.P.batch_size, (u64)h.P.idx_mini_batch))
		ranges.emplace_back(rg);                                // index.c:244,311-316 and bseq.c:86-98 on the record lengths
	if (log) fprintf(log, "[lqcov] parsed %zu target sequence(s) from the mapped file in %.3f s (%zu pieces, %u parsed again in order), %zu part(s)\n",
	                 flat.size(), lq_now_s() - t_parse0, recs.pieces.size(), recs.reparsed, ranges.size());
}

// the next part into hp[slot]
void TargetHost::produce(int slot)
{
	LQ_HIP_CHECK(hipSetDevice(h.device));                         // (may run on a thread of its own: page-locked allocations)
	const double tp0 = lq_now_s();
	struct Tm { double &t; double t0; ~Tm() { t = lq_now_s() - t0; } } tm{t_host[slot], tp0};
	HostPart &p = hp[slot];
	p.bs.clear(); p.n = 0; p.bases = 0; p.lens.clear(); p.names.clear(); p.name_off.assign(1, 0); p.last = false; p.any_amb.store(false);
	p.packed = mem;
	if (mem) produce_packed(p, t_alloc[slot]);
	else produce_streamed(p);
}

// One part = mini-batches of `chunk` bases while the running total is <= -I (index.c:244,311-316)
void TargetHost::produce_streamed(HostPart &p)
{
	u64 sum_len = 0;
	for (;;) {
		if (sum_len > h.P.batch_size) break;
		p.bs.emplace_back();
		if (ft->read_minibatch(chunk, p.bs.back(), false) == 0) { p.bs.pop_back(); p.last = true; break; }
		sum_len += p.bs.back().bases();
	}
	for (ReadBatch &b : p.bs) p.bases += b.bases();
}

void TargetHost::produce_packed(HostPart &p, double &t_alloc_slot)
{
	if (next_range >= ranges.size()) { p.last = true; return; }
	const size_t r0 = ranges[next_range].first, r1 = ranges[next_range].second;
	++next_range;
	p.last = next_range >= ranges.size();
	p.n = (u32)(r1 - r0);
	p.lens.resize(p.n);
	std::vector<u64> coff(p.n + 1, 0);
	u64 name_bytes = 0;
	for (u32 i = 0; i < p.n; ++i) { const FlatRec &r = flat[r0 + i]; p.lens[i] = r.seq_len; coff[i + 1] = coff[i] + ((u64)r.seq_len + LQ_CHUNK - 1) / LQ_CHUNK; p.bases += r.seq_len; name_bytes += r.name_len + 1; }
	const u64 n_words = coff[p.n] * LQ_CHUNK_WORDS;
	const double ta0 = lq_now_s();
	if (n_words > p.cap_words) {
		if (p.codes) hipHostFree(p.codes);
		if (p.amb) hipHostFree(p.amb);
		p.codes = nullptr; p.amb = nullptr;
		p.cap_words = n_words + n_words / 16 + 64;
		LQ_HIP_CHECK(hipHostMalloc((void**)&p.codes, p.cap_words * 8, 0));
		LQ_HIP_CHECK(hipHostMalloc((void**)&p.amb, p.cap_words * 4, 0));
		t_alloc_slot = lq_now_s() - ta0;
	}
	p.names.resize(name_bytes); p.name_off.resize(p.n + 1);
	{ u64 o = 0; for (u32 i = 0; i < p.n; ++i) { const FlatRec &r = flat[r0 + i]; p.name_off[i] = o; memcpy(p.names.data() + o, r.name, r.name_len); p.names[o + r.name_len] = 0; o += r.name_len + 1; } p.name_off[p.n] = o; }
	pack_reads(p, r0, coff);
}

// pack, read by read, equal shares of bases per thread
void TargetHost::pack_reads(HostPart &p, size_t r0, const std::vector<u64> &coff)
{
	const int nt = h.K.parse_threads > 0 ? h.K.parse_threads : (int)std::min<unsigned>(64, std::max(1u, std::thread::hardware_concurrency()));
	std::atomic<u32> next(0);
	auto work = [&]() {
		for (;;) {
			const u32 i0 = next.fetch_add(64);
			if (i0 >= p.n) break;
			for (u32 i = i0; i < std::min<u32>(i0 + 64, p.n); ++i) {
				const FlatRec &r = flat[r0 + i];
				const u64 off[2] = {0, r.seq_len};
				lq_pack_host(1, r.seq, off, p.codes + coff[i] * LQ_CHUNK_WORDS, p.amb + coff[i] * LQ_CHUNK_WORDS, 1);
				if (!p.any_amb.load(std::memory_order_relaxed) && lq_packed_read_ambiguous(p.amb + coff[i] * LQ_CHUNK_WORDS, r.seq_len)) p.any_amb.store(true);
			}
		}
	};
	if (nt <= 1 || p.n < 256) work();
	else { std::vector<std::thread> th; for (int t = 0; t < nt; ++t) th.emplace_back(work); for (auto &t : th) t.join(); }
}

// ---- sequences as the target: the parts ---------------------------------------------------------------------
// The parts go through a pipeline of three stages that overlap: the host makes part k + 2 (TargetHost), the build stream uploads,
// sketches and indexes part k + 1, the lanes map part k.  (-d and the index-only call keep one part at a time.)
struct PartRun {
	lqcov_handle &h;
	TargetHost &th;
	FILE *dump, *log;
	Part *dev[2];                                              // the part of slot 0 / 1 on the device
	int n_built = 0;
	std::future<void> host;                                    // the host at work on the next part

	void build(int slot);
	bool advance(int nxt);
};

// upload + sketch + index of hp[slot] (the build stream)
void PartRun::build(int slot)
{
	HostPart &p = th.hp[slot];
	Part &pt = *dev[slot];
	pt.clear(); pt.live = true;                                 // (a Part object is used again)
	const double tb0 = lq_now_s();
	if (p.packed) h.add_reads_packed(pt.rs, p.n, p.codes, p.any_amb.load() || h.K.upload_amb ? p.amb : nullptr, p.lens.data(), p.names.data(), p.name_off.data());   // (a part without an N: the codes alone cross PCIe)
	else for (ReadBatch &tb : p.bs) { h.add_reads(pt.rs, tb.size(), tb.seq.data(), tb.seq_off.data(), tb.names.data(), tb.name_off.data()); tb = ReadBatch(); }
	const double tu = lq_now_s();
	h.sketch(pt.rs, true);
	const double ts = lq_now_s();
	h.build_index(pt);
	if (log) fprintf(log, "[lqcov] part %d: %u target sequence(s), %" PRIu64 " bases, %" PRIu64 " minimizers, %" PRIu64 " distinct, mid_occ = %d  (host %.3f s of which page-locked allocation %.3f, upload %.3f s, sketch %.3f s, index %.3f s)\n",
	                 n_built, pt.rs.n, pt.rs.n_bases, pt.rs.n_mini, pt.n_keys, h.mid_occ, th.t_host[slot], th.t_alloc[slot], tu - tb0, ts - tu, lq_now_s() - ts);
	++n_built;
	if (dump) h.dump_part(pt, dump);                            // mm_idx_reader_read (index.c:533)
}

// the part of slot nxt from the host, then the host starts on the one after it; false: there was none
bool PartRun::advance(int nxt)
{
	LQ_HIP_CHECK(hipSetDevice(h.device));                         // (may run on a thread of its own)
	if (!host.valid()) return false;
	host.get();
	if (th.hp[nxt].empty()) return false;
	build(nxt);
	if (!th.hp[nxt].last) host = std::async(std::launch::async, &TargetHost::produce, &th, nxt ^ 1);   // (the other slot: uploaded long ago)
	return true;
}

void run_target_parts(lqcov_handle &h, const char *target, bool has_query, std::future<void> &queries_loaded, FILE *dump, FILE *log)
{
	const int64_t chunk = (int)((u64)h.P.idx_mini_batch < h.P.batch_size ? (u64)h.P.idx_mini_batch : h.P.batch_size);   // index.c:316
	TargetHost th(h, chunk);
	th.open(target, log);
#ifndef LQ_EMU
	const bool pipeline = h.K.pipeline && has_query && !dump && h.profiling != 1;
#else
	const bool pipeline = false;                                // (the test emulator runs one kernel at a time, on the calling thread)
#endif
	h.parts.emplace_back(new Part()); h.parts.emplace_back(new Part());
	PartRun run{h, th, dump, log, { h.parts[h.parts.size() - 2].get(), h.parts[h.parts.size() - 1].get() }};
	th.produce(0);
	if (queries_loaded.valid()) queries_loaded.get();          // (a query file that cannot be read: reported here)
	if (!th.hp[0].empty()) {
		if (!th.hp[0].last) run.host = std::async(std::launch::async, &TargetHost::produce, &th, 1);
		run.build(0);
		// the lanes size their work space from what is free when the first part stands: leave room for the part that is built meanwhile
		if (pipeline && !th.hp[0].last && h.hbm_reserve == 0) h.hbm_reserve = (u64)((double)std::min<u64>(th.hp[0].bases, h.P.batch_size + (u64)chunk) * 9.5);
		for (int k = 0;; ++k) {
			const int cur = k & 1, nxt = cur ^ 1;
			std::future<bool> next_ready;                         // part k + 1 built while part k is mapped
			if (pipeline) next_ready = std::async(std::launch::async, &PartRun::advance, &run, nxt);
			if (has_query) map_part_logged(h, *run.dev[cur], k, log);
			const bool more = pipeline ? next_ready.get() : run.advance(nxt);
			if (!more) break;
		}
		if (run.host.valid()) run.host.get();
	}
	for (Part *d : run.dev) for (auto &up : h.parts) if (up.get() == d) up.reset();
}

// ---- the end of the run ---------------------------------------------------------------------------------------
void finish_and_write(lqcov_handle &h, FILE *out, const lqcov_handle::QuerySetFiles *sets, FILE *log, double t_run0)
{
	const double tf0 = lq_now_s();
	h.finish();
	if (sets) for (size_t f = 0; f < sets->outs.size(); ++f) h.write_table_set((u32)f, sets->outs[f]);
	else h.write_table(out);
	if (log) fprintf(log, "[lqcov] rows and table in %.3f s; the whole call %.3f s (device allocations of this process so far: %.3f s for %.1f GB)\n", lq_now_s() - tf0, lq_now_s() - t_run0,
	                 (double)lq_alloc_ns * 1e-9, (double)lq_alloc_bytes * 1e-9);
}

// A uint16 match counter that reaches 65535 makes the reference's result depend on the order in which it processed the
// chains (esterr.c:130,136 test a[st], not a[j]).  Such a query's counters were replayed in that order (sat_replay_part) and its
// row is the reference's; only counters that reached the limit after being summed over ranks (accum_import) cannot be, and
// then the run says so and does not report success.
void report_saturated(lqcov_handle &h, FILE *log)
{
	u32 n_sat = 0, n_rep = 0;
	for (u32 i = 0; i < h.q.n; ++i) if (h.rows[i].flags & LQCOV_ROW_SATURATED) {
		if (h.rows[i].flags & LQCOV_ROW_REPLAYED) { ++n_rep; continue; }
		if (log && n_sat < 10) fprintf(log, "[WARNING] query %s: a match counter reached 65535 (esterr.c:130,136) in counters merged from several ranks: its row is not guaranteed to equal the reference's\n", h.q.names[h.q_inv[i]].c_str());
		++n_sat;
	}
	if (log && n_rep) fprintf(log, "[lqcov] %u quer%s with a match counter at its 16-bit limit (esterr.c:130,136): %llu chains replayed in the reference's order\n", n_rep, n_rep == 1 ? "y" : "ies", (unsigned long long)h.stat_sat_chains);
	if (n_sat) throw std::domain_error(std::to_string(n_sat) + " quer" + (n_sat == 1 ? "y" : "ies") + " with a saturated uint16 match counter (esterr.c:130,136) in merged counters: table written, rows flagged LQCOV_ROW_SATURATED without LQCOV_ROW_REPLAYED are not guaranteed");
}

} // namespace

int lqcov_handle::run_files(const char *target, const char *query, FILE *out, FILE *log, const char *dump_path, const QuerySetFiles *sets)
{
	if (sets) query = nullptr;
	const bool has_query = query || sets;
	const TargetProbe tp = probe_target(target);
	if (tp.is_idx && dump_path) throw std::domain_error("-d with a prebuilt index as the target is not supported");
	const double t_run0 = lq_now_s();
	std::future<void> queries_loaded;
	if (has_query) queries_loaded = start_queries(*this, query, sets, log, t_run0, !tp.is_idx);
	QueriesJoin queries_join{queries_loaded};
	FILE *dump = nullptr;
	if (dump_path) { dump = fopen(dump_path, "wb"); if (!dump) throw lq_open_error(dump_path); }
	Closer dump_closer{dump};
	if (tp.is_idx) run_prebuilt_parts(*this, target, tp.hdr, has_query, log);
	else run_target_parts(*this, target, has_query, queries_loaded, dump, log);
	if (!has_query) return 0;                                         // index only (minimap2-coverage.c:460-468)
	finish_and_write(*this, out, sets, log, t_run0);
	report_saturated(*this, log);
	return 0;
}
