// longqc_amd/csrc/reader.cpp -- the chunk loop's source behind the C ABI of include/lqcov.h (lqreader_*): what lq_utils.open_seq_chunk /
// parse_fastx_chunk (lq_utils.py:263-289, pysam.FastxFile = kseq) yield for a plain or gzip FASTA/FASTQ file, as resident chunks.
// The file is read (pread) or inflated (zlib) into a page-locked piece; the piece is parsed in place, record by record, into
// descriptors -- the name, the line segments of the sequence and of the quality string -- and uploaded as it is: the host looks at
// every byte once and copies none of the bases (what is copied is the one record that straddles the end of a piece: it moves to the
// front of the piece before the next read fills the rest).  k_chunk_gather (kernels_gather.hpp) then makes the chunk's flat sequence
// and quality buffers on the device, upper-casing the sequence if asked and giving records without a quality string '!'.
//
// The record grammar is kseq's, as fastx.hpp and fastx_mem.hpp state it; here the parser may stand at the end of what has been read
// so far and not at the end of the file, so it parses one record at a time and gives up (to be called again with more bytes) wherever
// kseq would have read on.  The chunk rule is parse_fastx_chunk's: size += getsizeof(name) + getsizeof(seq) + getsizeof(qual), a
// chunk ends with the record that makes size >= chunk_size; for an ASCII str getsizeof is str_overhead + len.
//
// A BAM file (file_code 0 of open_seq_chunk, parse_bam_chunk, lq_utils.py:238-261) goes through the same calls.  Its BGZF blocks are
// inflated into the piece by a pool of threads (bgzf.hpp); the host walks the records there and reads of each one the 36 fixed bytes
// and the name -- no base, no quality, no tag -- and hands k_bam_gather (kernels_bam.hpp) one descriptor per read for the packed
// sequence.  Every record is a read, whatever its flag; the qualities are '!' (open_seq_chunk passes is_sequel=True), or with
// lqreader_bam_qualities(r, 1) the file's, as chr(q + 33).  The chunk rule is the same sum.  The format is the SAM/BAM specification's
// (4.1 BGZF, 4.2 the records); no file here was read or written by htslib.
//
// lqreader_inflate(r, LQREADER_INFLATE_DEVICE): the BGZF blocks are inflated by k_bgzf_inflate (kernels_inflate.hpp) instead.  Only the
// compressed bytes go up; the kernel writes into the chunk's raw device buffer where the piece's upload would have put the bytes, and
// they come back into the piece for the host to parse and to check their CRC32.  The raw buffer then mirrors the piece from up_from to
// fill.  A bgzip FASTA/FASTQ is inflated the same way, any other gzip file by speculative spans (gzip.hpp, kernels_gzip.hpp).
//
// lqreader_host_copy(r, LQREADER_HOSTCOPY_NEEDED), for a FASTA/FASTQ file that the device both inflates and parses: the inflated bytes
// stay in the raw buffer.  k_crc32_ranges (kernels_crc32.hpp) makes the members' CRC32 there, k_fx_names (kernels_fxscan.hpp) the names
// of the records the scan vouches for, and the piece on the host holds only what host_bytes() has fetched: buf[v_lo .. v_hi), brought
// up to [pos - 1, fill) whenever parse_one is about to look.
//
// lqreader_bam_walk(r, LQREADER_BAMWALK_DEVICE), for a BAM file: the records of a piece are found on the device (bamscan.hpp,
// kernels_bamscan.hpp) wherever it vouches for them -- unaligned records that are whole inside the piece -- through DeviceParse's loop,
// and parse_bam_one takes what the device leaves; with lqreader_inflate's device mode lqreader_host_copy is then active for the BAM
// too.
//
// The parts: a Source (pread, gzread, BGZF blocks or gzip spans, chosen once) fills the Piece; parse_one, parse_bam_one (BamHeader) or
// DeviceParse (fxscan.hpp) finds the records, and each joins the chunk through ChunkParts::append_read: names, offsets, counts, the
// chunk rule.  What a Source finds wrong with its file is an lq_file_error; read_more gives it the path (LQCOV_E_IO by type).
#include "chunk.hpp"
#include "fastx_mem.hpp"
#include "bgzf.hpp"
#include "kernels_inflate.hpp"
#include "kernels_crc32.hpp"
#include "gzip.hpp"
#include "fxscan.hpp"
#include "bamscan.hpp"
#include <zlib.h>
#include <cstdlib>
#include <memory>

namespace {
thread_local std::string g_reader_open_error;

struct Line { u64 at; u64 len; };                             // bytes of the piece

struct Record {
	u64 name_at = 0, name_len = 0, seq_len = 0;
	bool has_qual = false;
	std::vector<Line> seq, qual;
};

enum { REC = 0, NEED_MORE = 1, END = 2, HDR = 3 };           // (HDR: parse_bam_one has put the BAM header behind it, nothing else)

// k_bgzf_inflate over host arrays: the compressed bytes go up, the kernel writes into d_out (16-byte aligned), the statuses come back
struct InflateDev {
	DBuf comp, jobs, status;
	void run(hipStream_t stream, const u8 *comp_host, u64 comp_len, const std::vector<InflateJob> &j, u8 *d_out, u32 *status_host)
	{
		const u32 n = (u32)j.size();
		if (!n) return;
		comp.ensure((size_t)(comp_len + 3) / 4 * 4 + LQ_INFLATE_PAD); jobs.ensure((size_t)n * sizeof(InflateJob)); status.ensure((size_t)n * 4);
		if (comp_len) LQ_HIP_CHECK(hipMemcpyAsync(comp.p, comp_host, (size_t)comp_len, hipMemcpyHostToDevice, stream));
		LQ_HIP_CHECK(hipMemcpyAsync(jobs.p, j.data(), (size_t)n * sizeof(InflateJob), hipMemcpyHostToDevice, stream));
		const u32 grid = std::min<u32>(n, LQ_INFLATE_MAX_BLOCKS);
		LQ_LAUNCH(k_bgzf_inflate, grid, LQ_INFLATE_THREADS, stream, comp.as<u8>(), jobs.as<InflateJob>(), n, d_out, status.as<u32>());
		LQ_HIP_CHECK(hipGetLastError());
		LQ_HIP_CHECK(hipMemcpyAsync(status_host, status.p, (size_t)n * 4, hipMemcpyDeviceToHost, stream));
		LQ_HIP_CHECK(hipStreamSynchronize(stream));
	}
};

// ---- where the bytes come from ----
// fill: bytes into dst[0 .. room) -> how many.  0 with `ended`: the file is over; 0 without: the next bytes want *need bytes of room.  How
// much of the room one call fills is the source's own matter.  A read that fails, or a file that is not what it says it is, is an
// lq_file_error.
struct Source {
	int fd = -1;                                              // closed with the source (gzread's stream owns its own)
	bool ended = false;
	bool in_mirror = false;                                   // fill puts the bytes into the chunk's raw device buffer as well
	hipStream_t stream = nullptr;                             // the stream of the chunk that is being made
	const lqinflate_stats *stats = nullptr;
	virtual u64 fill(u8 *dst, u64 room, u64 *need) = 0;
	virtual ~Source() { if (fd >= 0) ::close(fd); }
};

struct PlainSource : Source {
	u64 at = 0;
	explicit PlainSource(int f) { fd = f; }
	u64 fill(u8 *dst, u64 room, u64 *) override
	{
		const ssize_t got = ::pread(fd, dst, (size_t)std::min<u64>(room, 1u << 30), (off_t)at);
		if (got < 0) throw lq_file_error("read error");
		ended = got == 0; at += (u64)got;
		return (u64)got;
	}
};

struct GzreadSource : Source {
	gzFile gz;
	explicit GzreadSource(gzFile g) : gz(g) { gzbuffer(gz, 1 << 20); }
	~GzreadSource() { gzclose(gz); }
	u64 fill(u8 *dst, u64 room, u64 *) override
	{
		const int got = gzread(gz, dst, (unsigned)std::min<u64>(room, 1u << 30));
		if (got < 0) throw lq_file_error("not a complete gzip stream");
		ended = got == 0;
		return (u64)got;
	}
};

struct BgzfSource : Source {                                  // whole blocks; the call that finds the file over brings nothing
	BgzfInflater z;
	BgzfSource(int f, int n_threads) { fd = z.fd = f; z.n_threads = n_threads; }
	u64 fill(u8 *dst, u64 room, u64 *need) override { const u64 got = z.fill(dst, room, need); ended = !got && z.ended; return got; }
};

struct SpanSource : Source {                                  // as gzread: until the room is full, the stream over, or broken
	GzipInflater z;
	explicit SpanSource(int f) { fd = z.fd = f; z.span_bytes = GzipInflater::span_bytes_env(); stats = &z.stats; in_mirror = true; }
	u64 fill(u8 *dst, u64 room, u64 *need) override
	{
		u64 out = 0;
		z.stream = stream;
		while (!z.done && out < room) {
			const u64 got = z.fill(dst + out, room - out, need);
			if (!got && !z.done) break;                           // (no room: the next call's, or with nothing made the caller's to make)
			out += got;
		}
		ended = z.done;
		return out;
	}
};

// ---- the piece: buf[0 .. fill) read, [pos ..) not parsed yet, [up_from .. pos) parsed and not uploaded yet ----
struct Piece {
	u8 *buf = nullptr; u64 cap = 0, fill = 0, pos = 0, up_from = 0;
	int last_char = 0;                                        // kseq's: the header character at pos - 1 has been consumed
	bool eof = false;                                         // nothing more to read
	~Piece() { if (buf) lqcov_host_free(buf); }
	void resize(u64 bytes)
	{
		u8 *nb = (u8*)lqcov_host_alloc(bytes);
		if (!nb) throw std::runtime_error("no page-locked memory for a piece of the file");
		if (fill) memcpy(nb, buf, fill);
		if (buf) lqcov_host_free(buf);
		buf = nb; cap = bytes;
	}
};

// ---- the chunk being made ----
struct ChunkParts {
	u64 chunk_size = 0, overhead = 49;                        // the chunk rule
	u64 n_seqs = 0, n_bases = 0;                              // of the file so far
	std::vector<char> names; std::vector<u64> name_off, off; std::vector<u32> lens;
	std::vector<GatherSeg> sseg, qseg;                        // the host parsers' segments (device parse: the run behind the device lists)
	DBuf raw; u64 raw_used = 0;
	DBuf d_sseg, d_qseg; u64 n_dss = 0, n_dqs = 0;            // device parse: the chunk's segments on the device
	u64 size = 0;

	void reset()
	{
		names.clear(); name_off.assign(1, 0); off.assign(1, 0); lens.clear(); sseg.clear(); qseg.clear();
		raw_used = n_dss = n_dqs = size = 0;
	}

	// one more read, whichever parser found it; true: the chunk rule ends the chunk with it
	// (ascii: the name is known to hold no byte of 0x80 or more)
	bool append_read(const u8 *name, u64 name_len, u64 seq_len, bool ascii = false)
	{
		if (lens.size() == 0xffffffffULL) throw std::domain_error("more than 2^32-1 reads in one chunk");
		for (u64 i = 0; i < name_len && !ascii; ++i) if (name[i] >= 0x80)
			throw std::domain_error("a read name holds a byte of 0x80 or more (read " + std::to_string(n_seqs + 1) + "): not ASCII");
		names.insert(names.end(), name, name + name_len); names.push_back('\0');
		name_off.push_back(names.size());
		off.push_back(off.back() + seq_len);
		lens.push_back((u32)seq_len);
		++n_seqs; n_bases += seq_len;
		size += 3 * overhead + name_len + 2 * seq_len;
		return size >= chunk_size;
	}

	// device room for `more` raw bytes behind raw_used, what is there -- and `keep` bytes behind raw_used -- kept
	void raw_reserve(hipStream_t stream, u64 more, u64 keep = 0)
	{
		const u64 need = raw_used + more + LQ_GATHER_SRC_PAD;
		raw.grow((size_t)need, (size_t)std::max<u64>(need, 2 * raw_used + LQ_GATHER_SRC_PAD), (size_t)(raw_used + keep), stream);
	}

	static void seg_room(hipStream_t stream, DBuf &b, u64 have, u64 more)
	{
		const size_t need = (size_t)(have + more + 1) * sizeof(GatherSeg), kept = (size_t)have * sizeof(GatherSeg);
		b.grow(need, std::max(need, 2 * kept), kept, stream);
	}

	// the segments the host parser's records have made go behind the chunk's device lists
	void flush_host_segs(hipStream_t stream)
	{
		if (sseg.empty() && qseg.empty()) return;
		seg_room(stream, d_sseg, n_dss, sseg.size()); seg_room(stream, d_qseg, n_dqs, qseg.size());
		if (!sseg.empty()) LQ_HIP_CHECK(hipMemcpyAsync(d_sseg.as<GatherSeg>() + n_dss, sseg.data(), sseg.size() * sizeof(GatherSeg), hipMemcpyHostToDevice, stream));
		if (!qseg.empty()) LQ_HIP_CHECK(hipMemcpyAsync(d_qseg.as<GatherSeg>() + n_dqs, qseg.data(), qseg.size() * sizeof(GatherSeg), hipMemcpyHostToDevice, stream));
		LQ_HIP_CHECK(hipStreamSynchronize(stream));
		n_dss += sseg.size(); n_dqs += qseg.size();
		sseg.clear(); qseg.clear();
	}
};

// ---- the BAM header (magic, l_text, text, n_ref, per reference l_name, name, l_ref): skipped as it comes, it may be longer than the piece ----
struct BamHeader {
	int state = 0; u64 skip = 0; u32 refs = 0;                // 0 magic and l_text, 1 the text, 2 n_ref, 3 l_name, 4 name and l_ref, 5 records
	static u32 le32(const u8 *p) { return (u32)p[0] | (u32)p[1] << 8 | (u32)p[2] << 16 | (u32)p[3] << 24; }
	// true: the records begin at pc.pos
	bool advance(Piece &pc)
	{
		for (;;) {
			const u64 have = pc.fill - pc.pos;
			const u8 *p = pc.buf + pc.pos;
			switch (state) {
			case 0: if (have < 8) return false; skip = le32(p + 4); pc.pos += 8; state = 1; break;
			case 1: case 4: {
				const u64 m = std::min(have, skip);
				pc.pos += m; skip -= m;
				if (skip) return false;
				if (state == 4) --refs;
				state = state == 1 ? 2 : refs ? 3 : 5;
				break;
			}
			case 2: if (have < 4) return false; refs = le32(p); pc.pos += 4; state = refs ? 3 : 5; break;
			case 3: if (have < 4) return false; skip = (u64)le32(p) + 4; pc.pos += 4; state = 4; break;
			default: return true;
			}
		}
	}
};

// ---- lqreader_parse(r, LQREADER_PARSE_DEVICE): the records of a piece are found on the device (fxscan.hpp) wherever it vouches for them ----
struct DeviceParse {
	BamScan fx; lqparse_stats pst = {0, 0, 0, 0, 0, 0};
	int bam = 0;                                              // 0: a FASTA/FASTQ file (fx.run); 1, 2: a BAM file without / with the file's qualities (fx.run_bam)
	bool bol = true;                                          // the byte at pos -- with last_char, the header character in front of it -- is a line's first
	u64 cur = 0, org = 0, seg_s = 0, seg_q = 0, base_d = 0;   // the last scan's rows from cur on wait for a chunk: the piece byte its positions count from, record cur's first segments and base
	bool fresh = true, scanned = false, fb_counted = false, fb_at_end = false;      // bytes have come since the last scan; this piece has been scanned; that scan counts as a fallback / would if more records followed
	u64 host_recs = 0, skip = 0, backoff = 0;                 // records the host parser has made since the last scan; scans that found nothing wait for 1, 2, 4 .. of them
	lqcopy_stats *names_dev = nullptr;                        // not null: the piece does not hold the rows' names, k_fx_names brings them (the owner's account)

	bool rows_waiting() const { return cur < fx.n_rows; }
	void on_bytes() { ++pst.pieces; fresh = true; scanned = false; }

	// the host parser has made a record: the fallback and back-off accounts
	void on_host_record(bool eof)
	{
		++pst.records_host; ++host_recs;
		if (skip) --skip;
		if (scanned && !fb_counted) { if (eof) fb_at_end = true; else { ++pst.fallbacks; fb_counted = true; } }
	}

	// the scan over buf[pos .. fill) if the parser stands at a clean start and the range has not been scanned from here; true: there are rows
	bool scan(hipStream_t stream, const Piece &pc, const ChunkParts &ck)
	{
		if (!bol || pc.pos >= pc.fill) return false;
		if (!fresh && !(host_recs && !skip)) return false;
		fresh = false; host_recs = 0;
		org = pc.up_from; cur = 0; seg_s = seg_q = base_d = 0;
		if (bam) fx.run_bam(stream, ck.raw.as<u8>() + ck.raw_used, pc.fill - pc.up_from, pc.pos - pc.up_from, bam == 2);
		else fx.run(stream, ck.raw.as<u8>() + ck.raw_used, pc.fill - pc.up_from, pc.pos - pc.up_from, pc.last_char);
		if (!fx.n_lines) return false;
		++pst.scans; pst.lines += fx.n_lines;
		if (fx.n_rows && fb_at_end) ++pst.fallbacks;              // (the scan before stopped in front of these)
		scanned = true; fb_counted = fb_at_end = false;
		if (!fx.n_rows) { backoff = backoff ? std::min<u64>(backoff * 2, 1u << 20) : 1; skip = backoff; return false; }
		backoff = skip = 0;
		if (names_dev) fx.names(stream, ck.raw.as<u8>() + ck.raw_used, fx.rows.as<FxRow>(), fx.n_rows);
		return true;
	}

	// the waiting rows join the chunk until the chunk rule ends it (true) or they are used up; their segments move behind the chunk's,
	// device to device
	bool take_rows(hipStream_t stream, Piece &pc, ChunkParts &ck)
	{
		const u64 dst0 = ck.off.back();
		bool ended = false;
		while (cur < fx.n_rows && !ended) {
			const FxRow &w = fx.h_rows[cur];
			if (names_dev) { ended = ck.append_read((const u8*)fx.h_names.data() + fx.h_name_off[cur], w.name_len, w.seq_len, cur < fx.first_bad); ++names_dev->names_device; }
			else ended = ck.append_read(pc.buf + org + w.name_at, w.name_len, w.seq_len);
			++cur;
			++pst.records_device;
		}
		ck.flush_host_segs(stream);
		u64 s1 = 0, q1 = 0;
		fx.seg_start(stream, cur, &s1, &q1);
		const u64 ns = s1 - seg_s, nq = q1 - seg_q;
		// a byte of the scan lies at org + its position in the piece, and a byte of the piece at raw_used - up_from + its place in the raw bytes
		const u64 src_add = ck.raw_used + org - pc.up_from, dst_add = dst0 - base_d;
		ChunkParts::seg_room(stream, ck.d_sseg, ck.n_dss, ns); ChunkParts::seg_room(stream, ck.d_qseg, ck.n_dqs, nq);
		const auto grid = [](u64 n) { return (u32)std::min<u64>((n + LQ_FXSCAN_THREADS - 1) / LQ_FXSCAN_THREADS, LQ_FXSCAN_MAX_BLOCKS); };
		if (ns) LQ_LAUNCH(k_fx_rebase, grid(ns), LQ_FXSCAN_THREADS, stream, (const GatherSeg*)fx.sseg.as<GatherSeg>() + seg_s, ns, src_add, dst_add, ck.d_sseg.as<GatherSeg>() + ck.n_dss);
		if (nq) LQ_LAUNCH(k_fx_rebase, grid(nq), LQ_FXSCAN_THREADS, stream, (const GatherSeg*)fx.qseg.as<GatherSeg>() + seg_q, nq, src_add, dst_add, ck.d_qseg.as<GatherSeg>() + ck.n_dqs);
		LQ_HIP_CHECK(hipGetLastError());
		ck.n_dss += ns; ck.n_dqs += nq; seg_s = s1; seg_q = q1;
		base_d += ck.off.back() - dst0;
		if (cur < fx.n_rows) { pc.pos = org + fx.h_rows[cur].name_at - (bam ? 36 : 1); pc.last_char = 0; }      // (the record's first byte)
		else { pc.pos = org + fx.resume_pos; pc.last_char = fx.resume_last_char; }
		bol = true;
		return ended;
	}
};
} // namespace

struct lqreader {
	std::string path, err;
	int device = 0, n_threads = 1;
	bool upper = true;
	int format = 0;                                           // 0 FASTA/FASTQ, 1 BAM
	bool gzip = false, bgzf_text = false;                     // the file begins with gzip's magic; it is BGZF and not BAM
	bool bam_qual = false;                                       // the qualities come from the file
	int inflate_mode = LQREADER_INFLATE_HOST, parse_mode = LQREADER_PARSE_HOST;   // lqreader_inflate's, lqreader_parse's
	int host_copy = LQREADER_HOSTCOPY_ALL;                    // lqreader_host_copy's
	int bam_walk = LQREADER_BAMWALK_HOST;                     // lqreader_bam_walk's
	bool keep = false;                                        // ... and it is active: the inflated bytes stay on the device
	u64 v_lo = 0, v_hi = 0;                                   // keep: buf[v_lo .. v_hi) is what the host holds of the piece
	lqcopy_stats cst = {0, 0, 0, 0, 0, 0};
	CrcDev crcdev; DBuf raw_next;
	bool started = false;                                     // lqreader_next has been called: the modes are final, and with them
	bool dev_parse = false, mirror = false;                   // ... the device parse is on; the raw buffer holds buf[up_from .. fill)
	bool over = false;                                        // no more records: the end of the file, or a truncated quality string (kseq: -2)
	bool done = false;                                        // the last chunk has been handed out
	std::unique_ptr<Source> src;
	InflateDev inf;
	Piece pc;
	BamHeader hdr; Record rec; DeviceParse dp;                // the parsers' state
	bool rec_ends = false;                                    // the record a host parser has just put into the chunk ends it
	ChunkParts ck;

	int open_fd() const
	{
		const int fd = ::open(path.c_str(), O_RDONLY);
		if (fd < 0) throw lq_open_error(path);
		return fd;
	}

	void open_file()
	{
		const int fd = open_fd();
		u8 magic[2] = {0, 0};
		gzip = ::pread(fd, magic, 2, 0) == 2 && magic[0] == 0x1f && magic[1] == 0x8b;
		const int kind = gzip ? bgzf_kind(fd) : 0;
		bgzf_text = kind == 1;
		if (kind == 2) { format = 1; src.reset(new BgzfSource(fd, n_threads)); }
		else if (gzip) {
			gzFile gz = gzdopen(fd, "r");                         // (the stream owns the descriptor now)
			if (!gz) { ::close(fd); throw lq_open_error(path); }
			src.reset(new GzreadSource(gz));
		}
		else src.reset(new PlainSource(fd));
	}

	// 2: a BGZF file whose first four inflated bytes are "BAM\1"; 1: another BGZF file (its first blocks inflate); 0: neither
	static int bgzf_kind(int fd)
	{
		try {
			BgzfInflater probe; probe.fd = fd;
			std::vector<u8> head(BgzfInflater::MAX_BLOCK + 4);
			u64 have = 0, need = 0;
			while (have < 4) {
				const u64 got = probe.fill(head.data() + have, BgzfInflater::MAX_BLOCK + 4 - have, &need, 1);
				if (!got) return 1;
				have += got;
			}
			return memcmp(head.data(), "BAM\1", 4) == 0 ? 2 : 1;
		} catch (const std::exception &) { return 0; }              // (not BGZF, or broken: gzread's to read or to refuse)
	}

	// the first lqreader_next: the modes are final, and the source is.  In device mode a BGZF file's blocks are inflated by the kernel and
	// any other gzip file by spans, from a descriptor of their own (nothing has been read through gzread's)
	void start()
	{
		started = true;
		dev_parse = format == 1 ? bam_walk == LQREADER_BAMWALK_DEVICE : parse_mode == LQREADER_PARSE_DEVICE;
		if (format == 1) { dp.bam = bam_qual ? 2 : 1; dp.bol = false; }      // (the scan waits for the header's end)
		keep = host_copy == LQREADER_HOSTCOPY_NEEDED && dev_parse && inflate_mode == LQREADER_INFLATE_DEVICE && gzip;
		cst.active = keep;
		if (keep) dp.names_dev = &cst;
		if (inflate_mode == LQREADER_INFLATE_DEVICE && (format == 1 || bgzf_text)) {
			if (format == 0) src.reset(new BgzfSource(open_fd(), n_threads));
			BgzfSource &b = static_cast<BgzfSource&>(*src);          // (a BAM file's source is one since open_file)
			b.in_mirror = true;
			b.z.device = [this](const std::vector<BgzfInflater::Block> &blocks, const u8 *win, u8 *dst, u64 out_bytes, std::vector<u32> &status) {
				const u8 *d_dst = mirror_at(dst, out_bytes);
				const u64 at = (u64)(d_dst - ck.raw.as<u8>()), lo = blocks.front().in & ~(u64)15, hi = blocks.back().in + blocks.back().in_len;
				std::vector<InflateJob> jobs(blocks.size());
				for (size_t i = 0; i < blocks.size(); ++i)
					jobs[i] = {blocks[i].in - lo, at + blocks[i].out, (u32)blocks[i].in_len, (u32)blocks[i].isize};
				status.assign(blocks.size(), 0);
				inf.run(src->stream, win + lo, hi - lo, jobs, ck.raw.as<u8>(), status.data());
				if (keep) {                                               // the bytes stay: their CRC32 comes instead
					std::vector<u64> off(blocks.size()), len(blocks.size());
					for (size_t i = 0; i < blocks.size(); ++i) { off[i] = at + blocks[i].out; len[i] = blocks[i].isize; }
					std::vector<u32> &crc = static_cast<BgzfSource&>(*src).z.dev_crc;
					crc.assign(blocks.size(), 0);
					crcdev.run(src->stream, ck.raw.as<u8>(), (u32)blocks.size(), off.data(), len.data(), crc.data());
					cst.bytes_crc_device += out_bytes;
					return;
				}
				if (out_bytes) LQ_HIP_CHECK(hipMemcpyAsync(dst, d_dst, (size_t)out_bytes, hipMemcpyDeviceToHost, src->stream));
				LQ_HIP_CHECK(hipStreamSynchronize(src->stream));
				cst.bytes_to_host += out_bytes; cst.bytes_crc_host += out_bytes;
			};
		} else if (inflate_mode == LQREADER_INFLATE_DEVICE && gzip) {
			SpanSource *s = new SpanSource(open_fd());
			src.reset(s);
			s->z.dev_room = [this](u8 *dst, u64 n) { return mirror_at(dst, n); };
			s->z.keep_on_device = keep; s->z.copied = &cst;
		}
		mirror = src->in_mirror || dev_parse;
	}

	// the place in the raw device buffer of the n bytes at dst, a place of the piece at or behind up_from: where upload() would put them.
	// Room is made, what lies in front of them is kept
	u8 *mirror_at(const u8 *dst, u64 n)
	{
		const u64 ahead = (u64)(dst - pc.buf) - pc.up_from;
		ck.raw_reserve(src->stream, ahead + n, ahead);
		return ck.raw.as<u8>() + ck.raw_used + ahead;
	}

	// n bytes of the piece at p go up to that place; the piece is free again
	void send_up(const u8 *p, u64 n)
	{
		LQ_HIP_CHECK(hipMemcpyAsync(mirror_at(p, n), p, (size_t)n, hipMemcpyHostToDevice, src->stream));
		LQ_HIP_CHECK(hipStreamSynchronize(src->stream));
	}

	// keep: what parse_one may look at -- the byte in front of pos and everything behind it -- comes from the mirror, as far as the
	// host does not hold it yet
	void host_bytes()
	{
		if (!keep) return;
		const u64 lo = pc.pos > pc.up_from ? pc.pos - 1 : pc.pos;
		if (lo < v_lo || lo > v_hi) v_lo = v_hi = lo;
		if (v_hi >= pc.fill) return;
		const u64 n = pc.fill - v_hi;
		LQ_HIP_CHECK(hipMemcpyAsync(pc.buf + v_hi, ck.raw.as<u8>() + ck.raw_used + (v_hi - pc.up_from), (size_t)n, hipMemcpyDeviceToHost, src->stream));
		LQ_HIP_CHECK(hipStreamSynchronize(src->stream));
		cst.bytes_to_host += n;
		v_hi = pc.fill;
	}

	// keep: a new chunk's mirror starts with the bytes behind the last chunk's, raw[from .. from + fill - up_from), which the host may not hold
	void move_mirror(u64 from)
	{
		const u64 n = pc.fill - pc.up_from;
		raw_next.ensure((size_t)(n + LQ_GATHER_SRC_PAD));            // (the two blocks take turns; raw_reserve grows the one in use)
		LQ_HIP_CHECK(hipMemcpyAsync(raw_next.p, ck.raw.as<u8>() + from, (size_t)n, hipMemcpyDeviceToDevice, src->stream));
		LQ_HIP_CHECK(hipStreamSynchronize(src->stream));
		ck.raw.swap(raw_next);
	}

	[[noreturn]] void bam_fail(const std::string &what) { throw lq_open_error(path, what); }

	// more bytes behind buf[fill); false: the file has ended
	bool read_more()
	{
		while (!pc.eof) {
			if (pc.fill == pc.cap) pc.resize(pc.cap * 2);             // a record longer than the piece
			u64 need = 0, got = 0;
			try { got = src->fill(pc.buf + pc.fill, pc.cap - pc.fill, &need); }
			catch (const lq_file_error &e) { bam_fail(e.what()); }      // (the file's, not the device's)
			if (got && mirror && !src->in_mirror) send_up(pc.buf + pc.fill, got);      // (device parse: the bytes go up as they come)
			if (src->in_mirror) cst.bytes_inflated += got;
			pc.fill += got;
			pc.eof = src->ended;
			if (got || pc.eof) return got != 0;
			pc.resize(std::max(pc.cap * 2, pc.fill + need));          // the next bytes want more room than there is behind what the piece holds
		}
		return false;
	}

	// kseq_read (kseq.h:184-224) on buf[pos .. fill): one record into `rec`.  NEED_MORE: the record may go on behind what has been
	// read, nothing is consumed but bytes in front of a header character; END: kseq returns -1 or -2.
	int parse_one()
	{
		const u8 *p = pc.buf; const u64 n = pc.fill; const bool eof = pc.eof;
		u64 &pos = pc.pos; int &last_char = pc.last_char;
		u64 q = pos; int lc = last_char;
		Record &r = rec;
		r.seq.clear(); r.qual.clear(); r.seq_len = 0; r.has_qual = false;
		if (lc == 0) {
			const u8 *h = MemFastx::next_header(p, q, n);
			if (!h) { pos = n; return eof ? END : NEED_MORE; }
			pos = (u64)(h - p);                                   // (what lies in front of a header character is never looked at again)
			q = pos + 1; lc = *h;
		}
		if (q >= n) { if (!eof) return NEED_MORE; pos = n; last_char = 0; return END; }      // the stream ends behind a header character: no record
		r.name_at = q;
		while (q < n && !MemFastx::is_space(p[q])) ++q;
		if (q == n && !eof) return NEED_MORE;
		r.name_len = q - r.name_at;
		if (q < n && p[q] != '\n') {                              // the comment
			const u8 *e = (const u8*)memchr(p + q, '\n', n - q);
			if (!e && !eof) return NEED_MORE;
			q = e ? (u64)(e - p) : n;
		}
		q = q < n ? q + 1 : n;
		int c = -1;
		for (;;) {                                                // sequence lines until a line that starts with '>', '@' or '+'
			if (q >= n) { if (!eof) return NEED_MORE; c = -1; break; }
			c = p[q++];
			if (c == '>' || c == '+' || c == '@') break;
			if (c == '\n') continue;
			const u64 l0 = q - 1;
			const u8 *e = (const u8*)memchr(p + q, '\n', n - q);
			if (!e && !eof) return NEED_MORE;
			const u64 l1 = e ? (u64)(e - p) : n;
			q = e ? l1 + 1 : n;
			r.seq.push_back({l0, l1 - l0}); r.seq_len += l1 - l0;
			// one trailing '\r' of the sequence so far is dropped after every line -- but for a line that is the file's last byte: kseq's
			// ks_getuntil2 returns at the end of the stream before it looks for the '\r' (kseq.h:98; fastx_mem.hpp has the same note)
			if (r.seq_len > 1 && p[l1 - 1] == '\r' && l0 + 1 != n) { --r.seq.back().len; --r.seq_len; }
		}
		if (r.seq_len > 0x7fffffffULL) throw std::domain_error("read longer than 2^31-1 bases (bseq.c:80)");
		if (c == '>' || c == '@') { pos = q; last_char = c; return REC; }
		if (c != '+') { pos = n; last_char = 0; return REC; }      // the end of the file: the last record (FASTA)
		{	// '+': the rest of that line is skipped
			const u8 *e = q < n ? (const u8*)memchr(p + q, '\n', n - q) : nullptr;
			if (!e) { if (!eof) return NEED_MORE; pos = n; last_char = 0; over = true; return END; }      // no quality string: kseq returns -2
			q = (u64)(e - p) + 1;
		}
		u64 qlen = 0;
		for (;;) {                                                // while (ks_getuntil2(qual, append) >= 0 && qual.l < seq.l)
			if (q >= n) { if (!eof) return NEED_MORE; break; }
			const u8 *e = (const u8*)memchr(p + q, '\n', n - q);
			if (!e && !eof) return NEED_MORE;
			const u64 l1 = e ? (u64)(e - p) : n;
			if (l1 > q) { r.qual.push_back({q, l1 - q}); qlen += l1 - q; }
			// kseq drops one trailing '\r' of the whole string so far, if that is longer than one character, after every line it appends
			// (an empty line after a line that ended in "\r\r" drops the second one)
			if (qlen > 1 && p[r.qual.back().at + r.qual.back().len - 1] == '\r') {
				if (--r.qual.back().len == 0) r.qual.pop_back();
				--qlen;
			}
			q = e ? l1 + 1 : n;
			if (qlen >= r.seq_len) break;
		}
		if (qlen != r.seq_len) { pos = n; last_char = 0; over = true; return END; }      // truncated quality: kseq returns -2, the stream ends
		pos = q; last_char = 0; r.has_qual = true;
		return REC;
	}

	// one BAM record at buf[pos ..) into the chunk.  NEED_MORE: the record is not whole in the piece yet; HDR (device walk): the header is over
	int parse_bam_one()
	{
		if (hdr.state != 5) {
			const bool in = hdr.advance(pc);
			if (mirror) ck.raw_used += pc.pos - pc.up_from;           // (the header is in the raw bytes already)
			pc.up_from = pc.pos;                                      // (no descriptor points into the header: it is not uploaded)
			if (!in) { if (pc.eof) bam_fail("the file ends inside the BAM header"); return NEED_MORE; }
			if (dev_parse) return HDR;                                // (the first record is the scan's to find like any other)
		}
		const u64 have = pc.fill - pc.pos;
		const std::string where = "BAM record " + std::to_string(ck.n_seqs + 1) + ": ";
		if (have == 0 && pc.eof) return END;
		if (have < 36) { if (pc.eof) bam_fail(where + "the file ends inside a record"); return NEED_MORE; }
		const u8 *p = pc.buf + pc.pos;
		const u64 block_size = BamHeader::le32(p), l_name = p[12], n_cigar = (u64)p[16] | (u64)p[17] << 8, l_seq = BamHeader::le32(p + 20);
		if (l_seq > 0x7fffffffULL) throw std::domain_error("read longer than 2^31-1 bases (bseq.c:80)");
		const u64 fields = 32 + l_name + 4 * n_cigar + (l_seq + 1) / 2 + l_seq;
		if (block_size > 0x7fffffffULL || block_size < fields)
			bam_fail(where + "block_size " + std::to_string((i32)block_size) + " is too small for its fields (" + std::to_string(fields) + " bytes)");
		if (l_name == 0) bam_fail(where + "l_read_name is 0");
		if (have < 4 + block_size) { if (pc.eof) bam_fail(where + "the file ends inside a record"); return NEED_MORE; }
		if (p[36 + l_name - 1] != 0) bam_fail(where + "the read name has no NUL at its end");
		// the packed sequence, the quality bytes behind it: up_from is the first byte of the next upload, which lands at raw_used
		const u64 packed = ck.raw_used - pc.up_from + pc.pos + 36 + l_name + 4 * n_cigar, d0 = ck.off.back();
		rec_ends = ck.append_read(p + 36, strlen((const char*)p + 36), l_seq);
		if (l_seq) {
			ck.sseg.push_back({packed, d0});
			ck.qseg.push_back({bam_qual ? packed + (l_seq + 1) / 2 : LQ_GATHER_FILL, d0});
		}
		pc.pos += 4 + block_size;
		return REC;
	}

	// parse_one's `rec` joins the chunk, with its segments
	void add_record()
	{
		const Record &r = rec;
		// where a byte of the piece lies in the chunk's raw bytes: up_from is the first byte of the next upload, which lands at raw_used
		const u64 in_raw = ck.raw_used - pc.up_from, d0 = ck.off.back();
		rec_ends = ck.append_read(pc.buf + r.name_at, r.name_len, r.seq_len);
		u64 d = d0;
		for (const Line &l : r.seq) if (l.len) { ck.sseg.push_back({in_raw + l.at, d}); d += l.len; }
		d = d0;
		if (r.has_qual) { for (const Line &l : r.qual) { ck.qseg.push_back({in_raw + l.at, d}); d += l.len; } }
		else if (r.seq_len) ck.qseg.push_back({LQ_GATHER_FILL, d});
	}

	// buf[up_from .. pos) goes behind the raw bytes of the chunk (the descriptors made so far already point there)
	void upload()
	{
		const u64 len = pc.pos - pc.up_from;
		if (len && !mirror) send_up(pc.buf + pc.up_from, len);    // (a mirror holds them already)
		ck.raw_used += len;
		pc.up_from = pc.pos;
	}

	// the record that straddles the piece's end moves to its front, the file goes on behind it
	void refill()
	{
		upload();
		if (pc.pos) memmove(pc.buf, pc.buf + pc.pos, (size_t)(pc.fill - pc.pos));      // (keep: parse_one has just seen these bytes)
		v_lo = v_lo > pc.pos ? v_lo - pc.pos : 0; v_hi = v_hi > pc.pos ? v_hi - pc.pos : 0;
		pc.fill -= pc.pos; pc.pos = 0; pc.up_from = 0;
		more();
	}

	void more() { if (read_more()) dp.on_bytes(); }

	// the next chunk into c: records until the chunk rule ends it, or until the file does (*last)
	void next(lqchunk &c, u32 *n_out, u64 *n_seqs_cum, u64 *n_bases_cum, int *last)
	{
		if (done) throw std::logic_error("the reader has handed out its last chunk");
		if (c.device != device) throw std::invalid_argument("the chunk lives on another device than the reader");
		lq_cabi::select_device(device);
		if (!c.stream) LQ_HIP_CHECK(hipStreamCreate(&c.stream));
		if (!started) start();
		src->stream = c.stream;
		c.resident = false; c.packed = false; c.n_chunks = 0;
		const u64 raw_end = ck.raw_used;                          // (behind the last chunk's raw bytes: the bytes of the piece that it left)
		ck.reset();
		if (!pc.buf) { pc.resize(piece_bytes()); more(); }
		else if (mirror && pc.fill > pc.up_from) {                // (the mirror starts anew)
			if (keep) move_mirror(raw_end);
			else send_up(pc.buf + pc.up_from, pc.fill - pc.up_from);
		}
		bool ended = false;
		while (!over && !ended) {
			if (dev_parse && (dp.rows_waiting() || dp.scan(c.stream, pc, ck))) { ended = dp.take_rows(c.stream, pc, ck); continue; }
			const u64 pos0 = pc.pos;
			host_bytes();
			const int st = format == 1 ? parse_bam_one() : parse_one();
			if (format == 1) dp.bol = hdr.state == 5;                 // (a BAM parser stands at a record boundary once the header is behind it)
			else if (st == REC) dp.bol = true;
			else if (pc.pos != pos0) dp.bol = pc.buf[pc.pos - 1] == '\n';
			if (st == NEED_MORE) { refill(); continue; }
			if (st == HDR) continue;
			if (st == END) { over = true; break; }
			if (dev_parse) dp.on_host_record(pc.eof);
			if (format == 0) add_record();
			ended = rec_ends;
		}
		if (dev_parse) ck.flush_host_segs(c.stream);
		upload();
		done = !ended;
		if (dev_parse) lq_chunk_gather_dev(c, ck.off, ck.raw.as<u8>(), ck.d_sseg.as<GatherSeg>(), ck.n_dss, ck.d_qseg.as<GatherSeg>(), ck.n_dqs, upper, dp.bam);
		else lq_chunk_gather(c, ck.off, ck.raw.as<u8>(), ck.sseg, ck.qseg, upper, format == 1 ? (bam_qual ? 2 : 1) : 0);
		*n_out = c.n; *n_seqs_cum = ck.n_seqs; *n_bases_cum = ck.n_bases; *last = done ? 1 : 0;
	}

	// LQREADER_PIECE_BYTES: the size of a piece (tests: pieces shorter than a record)
	static u64 piece_bytes()
	{
		const char *e = getenv("LQREADER_PIECE_BYTES");
		const u64 v = e ? strtoull(e, nullptr, 10) : 0;
		return v ? std::max<u64>(v, 16) : (u64)16 << 20;
	}
};

namespace {
// a call without a handle: the message is lqreader_last_error(NULL)'s
template <class F> int one_shot(F &&f)
{
	char msg[512] = {0};
	const int rc = lq_cabi::guarded(msg, sizeof(msg), f);
	if (rc) g_reader_open_error = msg;
	return rc;
}

} // namespace

// ---- k_bgzf_inflate for another byte loop (polread.cpp; the kernel is compiled in this file alone): the listed blocks of `win` are
// inflated to d_out + at + their .out, one status per block as BgzfInflater's device hook wants them.  Waits for the stream ----
struct LqDevInflate { InflateDev inf; };
LqDevInflate *lq_dev_inflate_new() { return new LqDevInflate(); }
void lq_dev_inflate_free(LqDevInflate *d) { delete d; }
void lq_dev_inflate_run(LqDevInflate *d, hipStream_t stream, const std::vector<BgzfInflater::Block> &blocks, const u8 *win, u8 *d_out, u64 at, std::vector<u32> &status)
{
	status.assign(blocks.size(), 0);
	if (blocks.empty()) return;
	const u64 lo = blocks.front().in & ~(u64)15, hi = blocks.back().in + blocks.back().in_len;
	std::vector<InflateJob> jobs(blocks.size());
	for (size_t i = 0; i < blocks.size(); ++i) jobs[i] = {blocks[i].in - lo, at + blocks[i].out, (u32)blocks[i].in_len, (u32)blocks[i].isize};
	d->inf.run(stream, win + lo, hi - lo, jobs, d_out, status.data());
}

extern "C" {

lqreader *lqreader_open(const char *path, int device, uint64_t chunk_size, int is_upper, uint32_t str_overhead, int n_threads)
{
	try {
		if (!path) throw std::invalid_argument("null path");
		lq_cabi::select_device(device);
		std::unique_ptr<lqreader> r(new lqreader());
		r->path = path; r->device = device; r->ck.chunk_size = chunk_size; r->upper = is_upper != 0; r->ck.overhead = str_overhead;
		r->n_threads = n_threads <= 0 ? 16 : std::min(n_threads, 16);
		const char *mode = getenv("LQREADER_INFLATE");
		if (mode && !strcmp(mode, "device")) r->inflate_mode = LQREADER_INFLATE_DEVICE;
		const char *pm = getenv("LQREADER_PARSE");
		if (pm && !strcmp(pm, "device")) r->parse_mode = LQREADER_PARSE_DEVICE;
		const char *bw = getenv("LQREADER_BAMWALK");
		if (bw && !strcmp(bw, "device")) r->bam_walk = LQREADER_BAMWALK_DEVICE;
		const char *hc = getenv("LQREADER_HOSTCOPY");
		if (hc && !strcmp(hc, "needed")) r->host_copy = LQREADER_HOSTCOPY_NEEDED;
		r->open_file();
		return r.release();
	} catch (const std::exception &e) { g_reader_open_error = e.what(); return nullptr; }
}

void lqreader_close(lqreader *r)
{
	if (!r) return;
	(void)hipSetDevice(r->device);
	delete r;
}

const char *lqreader_last_error(const lqreader *r) { return r ? r->err.c_str() : g_reader_open_error.c_str(); }

int lqreader_next(lqreader *r, lqchunk *c, uint32_t *n, uint64_t *n_seqs_cum, uint64_t *n_bases_cum, int *last)
{
	if (!r) return LQCOV_E_ARG;
	char buf[512] = {0};
	const int rc = lq_cabi::guarded(buf, sizeof(buf), [&] {
		if (!c || !n || !n_seqs_cum || !n_bases_cum || !last) throw std::invalid_argument("null arguments");
		r->next(*c, n, n_seqs_cum, n_bases_cum, last);
	});
	if (rc) { r->err = buf; r->done = true; }                 // (a reader that failed hands out nothing more)
	return rc;
}

int lqreader_format(const lqreader *r) { return r ? r->format : LQCOV_E_ARG; }

int lqreader_bam_qualities(lqreader *r, int from_file)
{
	if (!r) return LQCOV_E_ARG;
	if (r->started) { r->err = "lqreader_bam_qualities after the first lqreader_next"; return LQCOV_E_STATE; }
	r->bam_qual = from_file != 0;
	return 0;
}

int lqreader_inflate(lqreader *r, int mode)
{
	if (!r || (mode != LQREADER_INFLATE_HOST && mode != LQREADER_INFLATE_DEVICE)) return LQCOV_E_ARG;
	if (r->started) { r->err = "lqreader_inflate after the first lqreader_next"; return LQCOV_E_STATE; }
	r->inflate_mode = mode;
	return 0;
}

int lqreader_parse(lqreader *r, int mode)
{
	if (!r || (mode != LQREADER_PARSE_HOST && mode != LQREADER_PARSE_DEVICE)) return LQCOV_E_ARG;
	if (r->started) { r->err = "lqreader_parse after the first lqreader_next"; return LQCOV_E_STATE; }
	r->parse_mode = mode;
	return 0;
}

int lqreader_bam_walk(lqreader *r, int mode)
{
	if (!r || (mode != LQREADER_BAMWALK_HOST && mode != LQREADER_BAMWALK_DEVICE)) return LQCOV_E_ARG;
	if (r->started) { r->err = "lqreader_bam_walk after the first lqreader_next"; return LQCOV_E_STATE; }
	r->bam_walk = mode;
	return 0;
}

int lqreader_host_copy(lqreader *r, int mode)
{
	if (!r || (mode != LQREADER_HOSTCOPY_ALL && mode != LQREADER_HOSTCOPY_NEEDED)) return LQCOV_E_ARG;
	if (r->started) { r->err = "lqreader_host_copy after the first lqreader_next"; return LQCOV_E_STATE; }
	r->host_copy = mode;
	return 0;
}

int lqreader_copy_stats(const lqreader *r, lqcopy_stats *stats)
{
	if (!r || !stats) return LQCOV_E_ARG;
	*stats = r->cst;
	return 0;
}

int lqcrc32_ranges(int device, const uint8_t *bytes, uint64_t n_bytes, uint32_t n, const uint64_t *off, const uint64_t *len, uint32_t *crc_out)
{
	return one_shot([&] {
		if (!n) return;
		if (!off || !len || !crc_out || (n_bytes && !bytes)) throw std::invalid_argument("null buffers");
		for (u32 i = 0; i < n; ++i)
			if (off[i] > n_bytes || len[i] > n_bytes - off[i]) throw std::invalid_argument("a range lies outside the bytes");
		lq_cabi::ScopedStream stream(device);
		DBuf d;
		d.ensure((size_t)n_bytes + LQ_GATHER_SRC_PAD);
		if (n_bytes) LQ_HIP_CHECK(hipMemcpyAsync(d.p, bytes, (size_t)n_bytes, hipMemcpyHostToDevice, stream));
		CrcDev crc;
		crc.run(stream, d.as<u8>(), n, off, len, crc_out);
	});
}

int lqfx_names(int device, const uint8_t *bytes, uint64_t n, const uint32_t *rows, uint64_t n_rows, char *names_out, uint64_t names_cap,
               uint64_t *name_off_out, uint64_t *first_bad)
{
	return one_shot([&] {
		if (!name_off_out || !first_bad || (n && !bytes) || (n_rows && !rows)) throw std::invalid_argument("null buffers");
		name_off_out[0] = 0; *first_bad = n_rows;
		if (!n_rows) return;
		u64 blob = 0;
		for (u64 i = 0; i < n_rows; ++i) {
			if (rows[4 * i] > n || rows[4 * i + 1] > n - rows[4 * i]) throw std::invalid_argument("a name lies outside the bytes");
			blob += (u64)rows[4 * i + 1] + 1;
		}
		if (blob > names_cap || !names_out) throw std::invalid_argument("names_cap is smaller than the names");
		lq_cabi::ScopedStream stream(device);
		DBuf d, d_rows;
		d.ensure((size_t)n + LQ_GATHER_SRC_PAD); d_rows.ensure((size_t)n_rows * sizeof(FxRow));
		if (n) LQ_HIP_CHECK(hipMemcpyAsync(d.p, bytes, (size_t)n, hipMemcpyHostToDevice, stream));
		LQ_HIP_CHECK(hipMemcpyAsync(d_rows.p, rows, (size_t)n_rows * sizeof(FxRow), hipMemcpyHostToDevice, stream));
		FxScan fx;
		fx.names(stream, d.as<u8>(), (const FxRow*)d_rows.as<FxRow>(), n_rows);
		memcpy(names_out, fx.h_names.data(), fx.h_names.size());
		memcpy(name_off_out, fx.h_name_off.data(), (size_t)(n_rows + 1) * 8);
		*first_bad = fx.first_bad;
	});
}

int lqreader_parse_stats(const lqreader *r, lqparse_stats *stats)
{
	if (!r || !stats) return LQCOV_E_ARG;
	*stats = r->dp.pst;
	return 0;
}

int lqfx_scan(int device, const uint8_t *bytes, uint64_t n, uint64_t start_pos, int last_char, uint32_t *rows, uint64_t n_rows_cap,
              uint64_t *sseg, uint64_t *qseg, uint64_t seg_cap, uint64_t *n_rows, uint64_t *n_sseg, uint64_t *n_qseg,
              uint64_t *resume_pos, int *resume_last_char)
{
	return one_shot([&] {
		if (!n_rows || !n_sseg || !n_qseg || !resume_pos || !resume_last_char || (n && !bytes)) throw std::invalid_argument("null buffers");
		if (start_pos > n || (last_char != 0 && last_char != '@' && last_char != '>')) throw std::invalid_argument("no parser state");
		*n_rows = *n_sseg = *n_qseg = 0; *resume_pos = start_pos; *resume_last_char = last_char;
		// a clean start: at the first byte of a line, or behind a header character that was one (anything else is the host parser's)
		const uint64_t at = start_pos - (last_char ? 1 : 0);
		if (last_char && (start_pos == 0 || bytes[start_pos - 1] != last_char)) throw std::invalid_argument("no parser state");
		if ((at && bytes[at - 1] != '\n') || start_pos >= n) return;
		lq_cabi::ScopedStream stream(device);
		DBuf d;
		d.ensure((size_t)n + LQ_GATHER_SRC_PAD);
		LQ_HIP_CHECK(hipMemcpyAsync(d.p, bytes, (size_t)n, hipMemcpyHostToDevice, stream));
		FxScan fx;
		fx.run(stream, d.as<u8>(), n, start_pos, last_char);
		if (fx.n_rows > n_rows_cap || fx.n_sseg > seg_cap || fx.n_qseg > seg_cap) throw std::invalid_argument("the tables are smaller than the scan's result");
		if (fx.n_rows && (!rows || (fx.n_sseg && !sseg) || (fx.n_qseg && !qseg))) throw std::invalid_argument("null buffers");
		if (fx.n_rows) memcpy(rows, fx.h_rows.data(), (size_t)fx.n_rows * sizeof(FxRow));
		if (fx.n_sseg) LQ_HIP_CHECK(hipMemcpyAsync(sseg, fx.sseg.p, (size_t)fx.n_sseg * sizeof(GatherSeg), hipMemcpyDeviceToHost, stream));
		if (fx.n_qseg) LQ_HIP_CHECK(hipMemcpyAsync(qseg, fx.qseg.p, (size_t)fx.n_qseg * sizeof(GatherSeg), hipMemcpyDeviceToHost, stream));
		LQ_HIP_CHECK(hipStreamSynchronize(stream));
		*n_rows = fx.n_rows; *n_sseg = fx.n_sseg; *n_qseg = fx.n_qseg; *resume_pos = fx.resume_pos; *resume_last_char = fx.resume_last_char;
	});
}

int lqbam_scan(int device, const uint8_t *bytes, uint64_t n, uint64_t start_pos, int with_qual, uint32_t *rows, uint64_t n_rows_cap,
               uint64_t *sseg, uint64_t *qseg, uint64_t seg_cap, uint64_t *n_rows, uint64_t *n_sseg, uint64_t *n_qseg, uint64_t *resume_pos)
{
	return one_shot([&] {
		if (!n_rows || !n_sseg || !n_qseg || !resume_pos || (n && !bytes)) throw std::invalid_argument("null buffers");
		if (start_pos > n) throw std::invalid_argument("no parser state");
		*n_rows = *n_sseg = *n_qseg = 0; *resume_pos = start_pos;
		if (start_pos >= n) return;
		lq_cabi::ScopedStream stream(device);
		DBuf d;
		d.ensure((size_t)n + LQ_GATHER_SRC_PAD);
		LQ_HIP_CHECK(hipMemcpyAsync(d.p, bytes, (size_t)n, hipMemcpyHostToDevice, stream));
		BamScan bs;
		bs.run_bam(stream, d.as<u8>(), n, start_pos, with_qual != 0);
		if (bs.n_rows > n_rows_cap || bs.n_sseg > seg_cap || bs.n_qseg > seg_cap) throw std::invalid_argument("the tables are smaller than the scan's result");
		if (bs.n_rows && (!rows || (bs.n_sseg && !sseg) || (bs.n_qseg && !qseg))) throw std::invalid_argument("null buffers");
		if (bs.n_rows) memcpy(rows, bs.h_rows.data(), (size_t)bs.n_rows * sizeof(FxRow));
		if (bs.n_sseg) LQ_HIP_CHECK(hipMemcpyAsync(sseg, bs.sseg.p, (size_t)bs.n_sseg * sizeof(GatherSeg), hipMemcpyDeviceToHost, stream));
		if (bs.n_qseg) LQ_HIP_CHECK(hipMemcpyAsync(qseg, bs.qseg.p, (size_t)bs.n_qseg * sizeof(GatherSeg), hipMemcpyDeviceToHost, stream));
		LQ_HIP_CHECK(hipStreamSynchronize(stream));
		*n_rows = bs.n_rows; *n_sseg = bs.n_sseg; *n_qseg = bs.n_qseg; *resume_pos = bs.resume_pos;
	});
}

int lqreader_inflate_stats(const lqreader *r, lqinflate_stats *stats)
{
	if (!r || !stats) return LQCOV_E_ARG;
	*stats = r->src->stats ? *r->src->stats : lqinflate_stats{};
	return 0;
}

int lqinflate_gzip(int device, const uint8_t *comp, uint64_t comp_len, uint32_t span_bytes, uint8_t *out, uint64_t out_cap, uint64_t *out_len,
                   lqinflate_stats *stats)
{
	return one_shot([&] {
		if (!out_len || (comp_len && !comp) || (out_cap && !out)) throw std::invalid_argument("null buffers");
		if (span_bytes && (span_bytes < 1024 || span_bytes > (1u << 17) || (span_bytes & 15))) throw std::invalid_argument("span_bytes must be a multiple of 16 from 1024 to 131072");
		*out_len = 0;
		lq_cabi::ScopedStream stream(device);
		DBuf d_out;
		d_out.ensure((size_t)out_cap + 16);
		GzipInflater g;
		u8 none[1];
		g.mem = comp_len ? comp : none; g.mem_len = comp_len; g.stream = stream;
		g.span_bytes = span_bytes ? span_bytes : GzipInflater::span_bytes_env();
		g.dev_room = [&](u8 *dst, u64) { return d_out.as<u8>() + (dst - out); };
		u64 n = 0;
		try {
			while (!g.done) {
				u64 need = 0;
				const u64 got = g.fill(out + n, out_cap - n, &need);
				n += got;
				if (!got && !g.done) throw std::invalid_argument("out_cap is smaller than the inflated stream");
			}
		} catch (const GzipError &e) { throw lq_open_error("(memory)", e.what()); }
		*out_len = n;
		if (stats) *stats = g.stats;
	});
}

int lqinflate_blocks(int device, const uint8_t *comp, uint64_t comp_len, uint32_t n, const uint64_t *in_off, const uint32_t *in_len,
                     const uint64_t *out_off, const uint32_t *isize, uint8_t *out_host, uint32_t *status)
{
	return one_shot([&] {
		if (!n) return;
		if (!in_off || !in_len || !out_off || !isize || !status || (comp_len && !comp)) throw std::invalid_argument("null buffers");
		std::vector<InflateJob> jobs(n);
		u64 out_len = 0;
		for (u32 i = 0; i < n; ++i) {
			if (isize[i] > 65536) throw std::invalid_argument("ISIZE above 65536");
			if (in_len[i] >= 1u << 24 || in_off[i] > comp_len || in_len[i] > comp_len - in_off[i]) throw std::invalid_argument("a block's bytes lie outside the compressed buffer");
			if (out_off[i] > ((u64)1 << 40)) throw std::invalid_argument("an output offset above 2^40");
			jobs[i] = {in_off[i], out_off[i], in_len[i], isize[i]};
			out_len = std::max(out_len, out_off[i] + isize[i]);
		}
		if (out_len && !out_host) throw std::invalid_argument("null buffers");
		lq_cabi::ScopedStream stream(device);
		InflateDev inf; DBuf out;
		out.ensure((size_t)out_len + 16);
		if (out_len) LQ_HIP_CHECK(hipMemcpyAsync(out.p, out_host, (size_t)out_len, hipMemcpyHostToDevice, stream));
		inf.run(stream, comp, comp_len, jobs, out.as<u8>(), status);
		if (out_len) LQ_HIP_CHECK(hipMemcpyAsync(out_host, out.p, (size_t)out_len, hipMemcpyDeviceToHost, stream));
		LQ_HIP_CHECK(hipStreamSynchronize(stream));
	});
}

int lqreader_names(const lqreader *r, const char **names, const uint64_t **name_off, const uint32_t **lens)
{
	if (!r || !names || !name_off || !lens) return LQCOV_E_ARG;
	*names = r->ck.names.data(); *name_off = r->ck.name_off.data(); *lens = r->ck.lens.data();
	return 0;
}

} // extern "C"
