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
// compressed bytes go up; the kernel writes the inflated bytes into the chunk's raw device buffer where the piece's upload would have
// put them, and they come back into the piece for the host to parse and to check their CRC32 -- the parsers and the gather kernels
// are the same, the upload of the piece falls away.  The raw buffer then mirrors the piece from its first byte that is not part of
// the chunk yet (up_from) to its last (fill), not only what has been parsed.  In that mode a BGZF file that is not BAM (bgzip
// FASTA/FASTQ) is inflated the same way and parsed by the kseq grammar; gzread is not used for it.  A gzip file that is not BGZF
// is inflated by speculative spans (gzip.hpp, kernels_gzip.hpp) under the same rules: the bytes land in the raw buffer, come back
// into the piece, and what the file is or is not is what gzread says of it.
#include "chunk.hpp"
#include "fastx_mem.hpp"
#include "bgzf.hpp"
#include "kernels_inflate.hpp"
#include "gzip.hpp"
#include "fxscan.hpp"
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

enum { REC = 0, NEED_MORE = 1, END = 2 };

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
} // namespace

struct lqreader {
	std::string path, err;
	int device = 0;
	u64 chunk_size = 0, overhead = 49;
	bool upper = true;
	int n_threads = 1;
	// the file
	int fd = -1; gzFile gz = nullptr; u64 file_pos = 0;
	bool eof = false;                                         // nothing more to read
	bool over = false;                                        // no more records: the end of the file, or a truncated quality string (kseq: -2)
	bool done = false;                                        // the last chunk has been handed out
	// BAM
	int format = 0;                                           // 0 FASTA/FASTQ, 1 BAM
	bool bam_qual = false, started = false;                   // the qualities come from the file; lqreader_next has been called
	BgzfInflater bgzf;
	int inflate_mode = LQREADER_INFLATE_HOST; bool bgzf_text = false;     // lqreader_inflate's; a BGZF file that is not BAM
	int bgzf_fd = -1;                                         // device mode on such a file: the descriptor the blocks are read from
	InflateDev inf; hipStream_t inf_stream = nullptr;
	GzipInflater gzdev; int gzdev_fd = -1;                    // device mode on a gzip file that is not BGZF
	int hdr_state = 0; u64 hdr_skip = 0; u32 hdr_refs = 0;    // the BAM header: 0 magic and l_text, 1 the text, 2 n_ref, 3 l_name, 4 name and l_ref, 5 records
	// the piece: buf[0 .. fill) read, [pos ..) not parsed yet, [up_from .. pos) parsed and not uploaded yet
	u8 *buf = nullptr; u64 cap = 0, fill = 0, pos = 0, up_from = 0;
	int last_char = 0;                                        // kseq's: the header character at pos - 1 has been consumed
	u64 n_seqs = 0, n_bases = 0;
	// the chunk being made
	DBuf raw; u64 raw_used = 0;
	std::vector<GatherSeg> sseg, qseg;
	std::vector<char> names; std::vector<u64> name_off, off; std::vector<u32> lens;
	Record rec;
	// lqreader_parse(r, LQREADER_PARSE_DEVICE): the records of a piece are found on the device (fxscan.hpp) wherever it vouches for them
	int parse_mode = LQREADER_PARSE_HOST;
	bool bol = true;                                          // the byte at pos -- with last_char, the header character in front of it -- is a line's first
	FxScan fx; lqparse_stats pst = {0, 0, 0, 0, 0, 0};
	DBuf d_sseg, d_qseg; u64 n_dss = 0, n_dqs = 0;            // the chunk's segments on the device; sseg / qseg hold the host-parsed run behind them
	u64 fx_cur = 0, fx_org = 0, fx_s = 0, fx_q = 0, fx_d = 0; // the last scan's rows from fx_cur on wait for a chunk: the piece byte its positions count from, record fx_cur's first segments and base
	bool fresh = true, scanned = false, fb_counted = false, fb_at_end = false;      // bytes have come since the last scan; this piece has been scanned; that scan counts as a fallback / would if more records followed
	u64 host_recs = 0, skip = 0, backoff = 0;                 // records parse_one has made since the last scan; scans that found nothing wait for 1, 2, 4 .. of them

	~lqreader()
	{
		if (gz) gzclose(gz);
		if (fd >= 0) ::close(fd);
		if (bgzf_fd >= 0) ::close(bgzf_fd);
		if (gzdev_fd >= 0) ::close(gzdev_fd);
		if (buf) lqcov_host_free(buf);
	}

	void open_file()
	{
		fd = ::open(path.c_str(), O_RDONLY);
		if (fd < 0) throw std::runtime_error("failed to open file '" + path + "'");
		u8 magic[2] = {0, 0};
		const bool is_gz = ::pread(fd, magic, 2, 0) == 2 && magic[0] == 0x1f && magic[1] == 0x8b;
		const int kind = is_gz ? bgzf_kind() : 0;
		bgzf_text = kind == 1;
		if (kind == 2) {
			format = 1;
			bgzf = BgzfInflater(); bgzf.fd = fd; bgzf.n_threads = n_threads;
			return;
		}
		if (is_gz) {
			gz = gzdopen(fd, "r");
			if (!gz) throw std::runtime_error("failed to open file '" + path + "'");
			fd = -1;                                              // (the stream owns it now)
			gzbuffer(gz, 1 << 20);
		}
	}

	// 2: a BGZF file whose first four inflated bytes are "BAM\1"; 1: another BGZF file (its first blocks inflate); 0: neither
	int bgzf_kind()
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

	bool use_bgzf() const { return format == 1 || (bgzf_text && inflate_mode == LQREADER_INFLATE_DEVICE); }
	bool use_gzdev() const { return format == 0 && gz && !bgzf_text && inflate_mode == LQREADER_INFLATE_DEVICE; }
	bool on_device() const { return inflate_mode == LQREADER_INFLATE_DEVICE && (use_bgzf() || use_gzdev()); }
	bool parse_dev() const { return parse_mode == LQREADER_PARSE_DEVICE && format == 0; }
	bool mirror() const { return on_device() || parse_dev(); }            // the raw buffer holds buf[up_from .. fill), not only what has been parsed

	// the first lqreader_next: the mode is final
	void start()
	{
		started = true;
		if (!on_device()) return;
		if (use_gzdev()) {                                        // (gz keeps its descriptor; nothing has been read through it)
			gzdev_fd = ::open(path.c_str(), O_RDONLY);
			if (gzdev_fd < 0) throw std::runtime_error("failed to open file '" + path + "'");
			gzdev.fd = gzdev_fd; gzdev.span_bytes = GzipInflater::span_bytes_env();
			gzdev.dev_room = [this](u8 *dst, u64 n) {             // as below: dst is a place of the piece
				const u64 ahead = (u64)(dst - buf) - up_from;
				raw_reserve(inf_stream, ahead + n, ahead);
				return raw.as<u8>() + raw_used + ahead;
			};
			return;
		}
		if (format == 0) {                                        // (gz keeps its descriptor; nothing has been read through it)
			bgzf_fd = ::open(path.c_str(), O_RDONLY);
			if (bgzf_fd < 0) throw std::runtime_error("failed to open file '" + path + "'");
			bgzf = BgzfInflater(); bgzf.fd = bgzf_fd; bgzf.n_threads = n_threads;
		}
		bgzf.device = [this](const std::vector<BgzfInflater::Block> &blocks, const u8 *win, u8 *dst, u64 out_bytes, std::vector<u32> &status) {
			// dst is buf + fill: its place in the raw bytes is where upload() would put it
			const u64 ahead = (u64)(dst - buf) - up_from, lo = blocks.front().in & ~(u64)15, hi = blocks.back().in + blocks.back().in_len;
			raw_reserve(inf_stream, ahead + out_bytes, ahead);
			std::vector<InflateJob> jobs(blocks.size());
			for (size_t i = 0; i < blocks.size(); ++i)
				jobs[i] = {blocks[i].in - lo, raw_used + ahead + blocks[i].out, (u32)blocks[i].in_len, (u32)blocks[i].isize};
			status.assign(blocks.size(), 0);
			inf.run(inf_stream, win + lo, hi - lo, jobs, raw.as<u8>(), status.data());
			if (out_bytes) LQ_HIP_CHECK(hipMemcpyAsync(dst, raw.as<u8>() + raw_used + ahead, (size_t)out_bytes, hipMemcpyDeviceToHost, inf_stream));
			LQ_HIP_CHECK(hipStreamSynchronize(inf_stream));
		};
	}

	[[noreturn]] void bam_fail(const std::string &what) { throw std::runtime_error("failed to open file '" + path + "': " + what); }

	void set_piece(u64 bytes)
	{
		u8 *nb = (u8*)lqcov_host_alloc(bytes);
		if (!nb) throw std::runtime_error("no page-locked memory for a piece of the file");
		if (fill) memcpy(nb, buf, fill);
		if (buf) lqcov_host_free(buf);
		buf = nb; cap = bytes;
	}

	// more bytes behind buf[fill); false: the file has ended
	bool read_more()
	{
		if (use_bgzf()) {
			while (!eof) {
				u64 need = 0, got = 0;
				try { got = bgzf.fill(buf + fill, cap - fill, &need); }
				catch (const std::runtime_error &e) {
					if (strncmp(e.what(), "BGZF block", 10) && strcmp(e.what(), "read error")) throw;      // (the device's, not the file's)
					bam_fail(e.what());
				}
				if (got) { fill += got; return true; }
				if (bgzf.ended) { eof = true; break; }
				set_piece(std::max(cap * 2, fill + need));            // a block larger than the room behind what the piece holds
			}
			return false;
		}
		if (use_gzdev()) {                                        // as gzread: until the piece is full, the stream over, or broken
			bool any = false;
			while (!eof) {
				u64 need = 0, got = 0;
				gzdev.stream = inf_stream;
				try { got = gzdev.fill(buf + fill, cap - fill, &need); }
				catch (const GzipError &e) { bam_fail(e.what()); }
				catch (const std::runtime_error &e) { if (strcmp(e.what(), "read error")) throw; bam_fail(e.what()); }
				fill += got; any = any || got;
				if (gzdev.done) { eof = true; break; }
				if (fill == cap) break;
				if (!got) {
					if (any) break;                                       // (the next call makes room)
					set_piece(std::max(cap * 2, fill + need));            // a block larger than the room behind what the piece holds
				}
			}
			return any;
		}
		while (!eof && fill < cap) {
			const u64 want = std::min<u64>(cap - fill, 1u << 30);
			i64 got;
			if (gz) {
				got = gzread(gz, buf + fill, (unsigned)want);
				if (got < 0) throw std::runtime_error("failed to open file '" + path + "': not a complete gzip stream");
			} else {
				got = ::pread(fd, buf + fill, want, (off_t)file_pos);
				if (got < 0) throw std::runtime_error("failed to open file '" + path + "': read error");
			}
			if (got == 0) { eof = true; break; }
			if (mirror()) {                                       // (device parse: the bytes go up as they come)
				const u64 ahead = fill - up_from;
				raw_reserve(inf_stream, ahead + (u64)got, ahead);
				LQ_HIP_CHECK(hipMemcpyAsync(raw.as<u8>() + raw_used + ahead, buf + fill, (size_t)got, hipMemcpyHostToDevice, inf_stream));
				LQ_HIP_CHECK(hipStreamSynchronize(inf_stream));
			}
			fill += (u64)got; file_pos += (u64)got;
			return true;
		}
		return false;
	}

	// kseq_read (kseq.h:184-224) on buf[pos .. fill): one record into `rec`.  NEED_MORE: the record may go on behind what has been
	// read, nothing is consumed but bytes in front of a header character; END: kseq returns -1 or -2.
	int parse_one()
	{
		const u8 *p = buf; const u64 n = fill;
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

	static u32 le32(const u8 *p) { return (u32)p[0] | (u32)p[1] << 8 | (u32)p[2] << 16 | (u32)p[3] << 24; }

	// the BAM header (magic, l_text, text, n_ref, per reference l_name, name, l_ref) is skipped as it comes: it may be longer than
	// the piece.  true: the records begin at pos
	bool bam_header()
	{
		for (;;) {
			const u64 have = fill - pos;
			switch (hdr_state) {
			case 0: if (have < 8) return false; hdr_skip = le32(buf + pos + 4); pos += 8; hdr_state = 1; break;
			case 1: case 4: {
				const u64 m = std::min(have, hdr_skip);
				pos += m; hdr_skip -= m;
				if (hdr_skip) return false;
				if (hdr_state == 4) --hdr_refs;
				hdr_state = hdr_state == 1 ? 2 : hdr_refs ? 3 : 5;
				break;
			}
			case 2: if (have < 4) return false; hdr_refs = le32(buf + pos); pos += 4; hdr_state = hdr_refs ? 3 : 5; break;
			case 3: if (have < 4) return false; hdr_skip = (u64)le32(buf + pos) + 4; pos += 4; hdr_state = 4; break;
			default: return true;
			}
		}
	}

	// one BAM record at buf[pos ..) into the chunk's descriptors.  NEED_MORE: the record is not whole in the piece yet
	int parse_bam_one()
	{
		if (hdr_state != 5) {
			const bool in = bam_header();
			if (on_device()) raw_used += pos - up_from;           // (the header is in the raw bytes already)
			up_from = pos;                                        // (no descriptor points into the header: it is not uploaded)
			if (!in) { if (eof) bam_fail("the file ends inside the BAM header"); return NEED_MORE; }
		}
		const u64 have = fill - pos;
		const std::string where = "BAM record " + std::to_string(n_seqs + 1) + ": ";
		if (have == 0 && eof) return END;
		if (have < 36) { if (eof) bam_fail(where + "the file ends inside a record"); return NEED_MORE; }
		const u8 *p = buf + pos;
		const u64 block_size = le32(p), l_name = p[12], n_cigar = (u64)p[16] | (u64)p[17] << 8, l_seq = le32(p + 20);
		if (l_seq > 0x7fffffffULL) throw std::domain_error("read longer than 2^31-1 bases (bseq.c:80)");
		const u64 fields = 32 + l_name + 4 * n_cigar + (l_seq + 1) / 2 + l_seq;
		if (block_size > 0x7fffffffULL || block_size < fields)
			bam_fail(where + "block_size " + std::to_string((i32)block_size) + " is too small for its fields (" + std::to_string(fields) + " bytes)");
		if (l_name == 0) bam_fail(where + "l_read_name is 0");
		if (have < 4 + block_size) { if (eof) bam_fail(where + "the file ends inside a record"); return NEED_MORE; }
		if (p[36 + l_name - 1] != 0) bam_fail(where + "the read name has no NUL at its end");
		if (lens.size() == 0xffffffffULL) throw std::domain_error("more than 2^32-1 reads in one chunk");
		const u8 *nm = p + 36;
		const u64 name_len = strlen((const char*)nm);
		for (u64 i = 0; i < name_len; ++i) if (nm[i] >= 0x80)
			throw std::domain_error("a read name holds a byte of 0x80 or more (read " + std::to_string(n_seqs + 1) + "): not ASCII");
		names.insert(names.end(), nm, nm + name_len + 1);
		name_off.push_back(names.size());
		// (where a byte of the piece lies in the chunk's raw bytes: add_record)
		const u64 seq_at = raw_used + (pos + 36 + l_name + 4 * n_cigar - up_from), d = off.back();
		if (l_seq) {
			sseg.push_back({seq_at, d});
			qseg.push_back({bam_qual ? seq_at + (l_seq + 1) / 2 : LQ_GATHER_FILL, d});
		}
		off.push_back(d + l_seq);
		lens.push_back((u32)l_seq);
		++n_seqs; n_bases += l_seq;
		rec.name_len = name_len; rec.seq_len = l_seq;
		pos += 4 + block_size;
		return REC;
	}

	// device room for `more` raw bytes behind raw_used, what is there -- and `keep` bytes behind raw_used -- kept
	void raw_reserve(hipStream_t stream, u64 more, u64 keep = 0)
	{
		const u64 need = raw_used + more + LQ_GATHER_SRC_PAD;
		if (need <= raw.cap) return;
		DBuf nb;
		nb.ensure((size_t)std::max<u64>(need, 2 * raw_used + LQ_GATHER_SRC_PAD));
		if (raw_used + keep) {
			LQ_HIP_CHECK(hipMemcpyAsync(nb.p, raw.p, (size_t)(raw_used + keep), hipMemcpyDeviceToDevice, stream));
			LQ_HIP_CHECK(hipStreamSynchronize(stream));
		}
		raw.swap(nb);
		nb.release();
	}

	// buf[up_from .. pos) goes behind the raw bytes of the chunk (the descriptors made so far already point there)
	void upload(hipStream_t stream)
	{
		const u64 len = pos - up_from;
		if (mirror()) raw_used += len;                            // (they are there already)
		else if (len) {
			raw_reserve(stream, len);
			LQ_HIP_CHECK(hipMemcpyAsync(raw.as<u8>() + raw_used, buf + up_from, (size_t)len, hipMemcpyHostToDevice, stream));
			LQ_HIP_CHECK(hipStreamSynchronize(stream));           // the piece is free again
			raw_used += len;
		}
		up_from = pos;
	}

	// the record that straddles the piece's end moves to its front, the file goes on behind it
	void refill(hipStream_t stream)
	{
		upload(stream);
		if (pos) memmove(buf, buf + pos, (size_t)(fill - pos));
		fill -= pos; pos = 0; up_from = 0;
		if (fill == cap) set_piece(cap * 2);                      // a record longer than the piece
		more();
	}

	void more() { if (read_more()) { ++pst.pieces; fresh = true; scanned = false; } }

	// ---- the device parse ----
	static void seg_room(hipStream_t stream, DBuf &b, u64 have, u64 more)
	{
		const size_t need = (size_t)(have + more + 1) * sizeof(GatherSeg);
		if (need <= b.cap) return;
		DBuf nb;
		nb.ensure(std::max(need, 2 * (size_t)have * sizeof(GatherSeg)));
		if (have) {
			LQ_HIP_CHECK(hipMemcpyAsync(nb.p, b.p, (size_t)have * sizeof(GatherSeg), hipMemcpyDeviceToDevice, stream));
			LQ_HIP_CHECK(hipStreamSynchronize(stream));
		}
		b.swap(nb);
		nb.release();
	}

	// the segments parse_one's records have made go behind the chunk's device lists
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

	// the scan's records fx_cur .. e have joined the chunk, their first base at dst0: their segments move behind the chunk's, device to device
	void take_run(hipStream_t stream, u64 e, u64 dst0)
	{
		flush_host_segs(stream);
		u64 s1 = 0, q1 = 0;
		fx.seg_start(stream, e, &s1, &q1);
		const u64 ns = s1 - fx_s, nq = q1 - fx_q;
		// a byte of the scan lies at fx_org + its position in the piece, and a byte of the piece at raw_used - up_from + its place in the raw bytes
		const u64 src_add = raw_used + fx_org - up_from, dst_add = dst0 - fx_d;
		seg_room(stream, d_sseg, n_dss, ns); seg_room(stream, d_qseg, n_dqs, nq);
		const auto grid = [](u64 n) { return (u32)std::min<u64>((n + LQ_FXSCAN_THREADS - 1) / LQ_FXSCAN_THREADS, LQ_FXSCAN_MAX_BLOCKS); };
		if (ns) LQ_LAUNCH(k_fx_rebase, grid(ns), LQ_FXSCAN_THREADS, stream, (const GatherSeg*)fx.sseg.as<GatherSeg>() + fx_s, ns, src_add, dst_add, d_sseg.as<GatherSeg>() + n_dss);
		if (nq) LQ_LAUNCH(k_fx_rebase, grid(nq), LQ_FXSCAN_THREADS, stream, (const GatherSeg*)fx.qseg.as<GatherSeg>() + fx_q, nq, src_add, dst_add, d_qseg.as<GatherSeg>() + n_dqs);
		LQ_HIP_CHECK(hipGetLastError());
		n_dss += ns; n_dqs += nq; fx_s = s1; fx_q = q1;
	}

	// the scan over buf[pos .. fill) if the parser stands at a clean start and the range has not been scanned from here; true: there are rows
	bool scan(hipStream_t stream)
	{
		if (!bol || pos >= fill) return false;
		if (!fresh && !(host_recs && !skip)) return false;
		fresh = false; host_recs = 0;
		fx_org = up_from; fx_cur = 0; fx_s = fx_q = fx_d = 0;
		fx.run(stream, raw.as<u8>() + raw_used, fill - up_from, pos - up_from, last_char);
		if (!fx.n_lines) return false;
		++pst.scans; pst.lines += fx.n_lines;
		if (fx.n_rows && fb_at_end) ++pst.fallbacks;              // (the scan before stopped in front of these)
		scanned = true; fb_counted = fb_at_end = false;
		if (!fx.n_rows) { backoff = backoff ? std::min<u64>(backoff * 2, 1u << 20) : 1; skip = backoff; return false; }
		backoff = skip = 0;
		return true;
	}

	// the waiting rows join the chunk until the chunk rule ends it (true) or they are used up
	bool take_rows(hipStream_t stream, u64 &size)
	{
		const u64 dst0 = off.back();
		bool ended = false;
		while (fx_cur < fx.n_rows && !ended) {
			const FxRow &w = fx.h_rows[fx_cur];
			if (lens.size() == 0xffffffffULL) throw std::domain_error("more than 2^32-1 reads in one chunk");
			const u8 *nm = buf + fx_org + w.name_at;
			for (u64 i = 0; i < w.name_len; ++i) if (nm[i] >= 0x80)
				throw std::domain_error("a read name holds a byte of 0x80 or more (read " + std::to_string(n_seqs + 1) + "): not ASCII");
			names.insert(names.end(), nm, nm + w.name_len); names.push_back('\0');
			name_off.push_back(names.size());
			off.push_back(off.back() + w.seq_len);
			lens.push_back(w.seq_len);
			++n_seqs; n_bases += w.seq_len; ++pst.records_device;
			++fx_cur;
			size += 3 * overhead + w.name_len + 2 * (u64)w.seq_len;
			ended = size >= chunk_size;
		}
		take_run(stream, fx_cur, dst0);
		fx_d += off.back() - dst0;
		if (fx_cur < fx.n_rows) { pos = fx_org + fx.h_rows[fx_cur].name_at - 1; last_char = 0; }
		else { pos = fx_org + fx.resume_pos; last_char = fx.resume_last_char; }
		bol = true;
		return ended;
	}

	void add_record()
	{
		const Record &r = rec;
		const u8 *nm = buf + r.name_at;
		for (u64 i = 0; i < r.name_len; ++i) if (nm[i] >= 0x80)
			throw std::domain_error("a read name holds a byte of 0x80 or more (read " + std::to_string(n_seqs + 1) + "): not ASCII");
		names.insert(names.end(), nm, nm + r.name_len); names.push_back('\0');
		name_off.push_back(names.size());
		// where a byte of the piece lies in the chunk's raw bytes: up_from is the first byte of the next upload, which lands at raw_used
		u64 d = off.back();
		for (const Line &l : r.seq) if (l.len) { sseg.push_back({raw_used + (l.at - up_from), d}); d += l.len; }
		d = off.back();
		if (r.has_qual) { for (const Line &l : r.qual) { qseg.push_back({raw_used + (l.at - up_from), d}); d += l.len; } }
		else if (r.seq_len) qseg.push_back({LQ_GATHER_FILL, d});
		off.push_back(off.back() + r.seq_len);
		lens.push_back((u32)r.seq_len);
		++n_seqs; n_bases += r.seq_len;
	}

	// the next chunk into c: records until the chunk rule ends it, or until the file does (*last)
	void next(lqchunk &c, u32 *n_out, u64 *n_seqs_cum, u64 *n_bases_cum, int *last)
	{
		if (done) throw std::logic_error("the reader has handed out its last chunk");
		if (c.device != device) throw std::invalid_argument("the chunk lives on another device than the reader");
		lq_cabi::select_device(device);
		if (!c.stream) LQ_HIP_CHECK(hipStreamCreate(&c.stream));
		inf_stream = c.stream;
		if (!started) start();
		c.resident = false; c.packed = false; c.n_chunks = 0;
		raw_used = 0; sseg.clear(); qseg.clear(); names.clear(); name_off.assign(1, 0); off.assign(1, 0); lens.clear();
		n_dss = n_dqs = 0;
		if (!buf) { set_piece(piece_bytes()); more(); }
		else if (mirror() && fill > up_from) {                 // what the piece still holds belongs to this chunk: the mirror starts anew
			raw_reserve(c.stream, fill - up_from);
			LQ_HIP_CHECK(hipMemcpyAsync(raw.p, buf + up_from, (size_t)(fill - up_from), hipMemcpyHostToDevice, c.stream));
			LQ_HIP_CHECK(hipStreamSynchronize(c.stream));
		}
		u64 size = 0; bool ended = false;
		while (!over) {
			if (parse_dev()) {
				if (fx_cur < fx.n_rows || scan(c.stream)) {
					if (take_rows(c.stream, size)) { ended = true; break; }
					continue;
				}
			}
			const u64 pos0 = pos;
			const int st = format == 1 ? parse_bam_one() : parse_one();
			if (st == REC) bol = true;
			else if (pos != pos0) bol = buf[pos - 1] == '\n';
			if (st == NEED_MORE) { refill(c.stream); continue; }
			if (st == END) { over = true; break; }
			if (parse_dev()) {
				++pst.records_host; ++host_recs;
				if (skip) --skip;
				if (scanned && !fb_counted) { if (eof) fb_at_end = true; else { ++pst.fallbacks; fb_counted = true; } }
			}
			if (format == 0) {
				if (lens.size() == 0xffffffffULL) throw std::domain_error("more than 2^32-1 reads in one chunk");
				add_record();
			}
			size += 3 * overhead + rec.name_len + 2 * rec.seq_len;
			if (size >= chunk_size) { ended = true; break; }
		}
		if (parse_dev()) flush_host_segs(c.stream);
		upload(c.stream);
		done = !ended;
		if (parse_dev()) lq_chunk_gather_dev(c, off, raw.as<u8>(), d_sseg.as<GatherSeg>(), n_dss, d_qseg.as<GatherSeg>(), n_dqs, upper);
		else lq_chunk_gather(c, off, raw.as<u8>(), sseg, qseg, upper, format == 1 ? (bam_qual ? 2 : 1) : 0);
		const u32 n = c.n;
		*n_out = n; *n_seqs_cum = n_seqs; *n_bases_cum = n_bases; *last = done ? 1 : 0;
	}

	// LQREADER_PIECE_BYTES: the size of a piece (tests: pieces shorter than a record)
	static u64 piece_bytes()
	{
		const char *e = getenv("LQREADER_PIECE_BYTES");
		const u64 v = e ? strtoull(e, nullptr, 10) : 0;
		return v ? std::max<u64>(v, 16) : (u64)16 << 20;
	}
};

extern "C" {

lqreader *lqreader_open(const char *path, int device, uint64_t chunk_size, int is_upper, uint32_t str_overhead, int n_threads)
{
	try {
		if (!path) throw std::invalid_argument("null path");
		lq_cabi::select_device(device);
		std::unique_ptr<lqreader> r(new lqreader());
		r->path = path; r->device = device; r->chunk_size = chunk_size; r->upper = is_upper != 0; r->overhead = str_overhead;
		r->n_threads = n_threads <= 0 ? 16 : std::min(n_threads, 16);
		const char *mode = getenv("LQREADER_INFLATE");
		if (mode && !strcmp(mode, "device")) r->inflate_mode = LQREADER_INFLATE_DEVICE;
		const char *pm = getenv("LQREADER_PARSE");
		if (pm && !strcmp(pm, "device")) r->parse_mode = LQREADER_PARSE_DEVICE;
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

int lqreader_parse_stats(const lqreader *r, lqparse_stats *stats)
{
	if (!r || !stats) return LQCOV_E_ARG;
	*stats = r->pst;
	return 0;
}

int lqfx_scan(int device, const uint8_t *bytes, uint64_t n, uint64_t start_pos, int last_char, uint32_t *rows, uint64_t n_rows_cap,
              uint64_t *sseg, uint64_t *qseg, uint64_t seg_cap, uint64_t *n_rows, uint64_t *n_sseg, uint64_t *n_qseg,
              uint64_t *resume_pos, int *resume_last_char)
{
	char msg[512] = {0};
	const int rc = lq_cabi::guarded(msg, sizeof(msg), [&] {
		if (!n_rows || !n_sseg || !n_qseg || !resume_pos || !resume_last_char || (n && !bytes)) throw std::invalid_argument("null buffers");
		if (start_pos > n || (last_char != 0 && last_char != '@' && last_char != '>')) throw std::invalid_argument("no parser state");
		*n_rows = *n_sseg = *n_qseg = 0; *resume_pos = start_pos; *resume_last_char = last_char;
		// a clean start: at the first byte of a line, or behind a header character that was one (anything else is the host parser's)
		const uint64_t at = start_pos - (last_char ? 1 : 0);
		if (last_char && (start_pos == 0 || bytes[start_pos - 1] != last_char)) throw std::invalid_argument("no parser state");
		if ((at && bytes[at - 1] != '\n') || start_pos >= n) return;
		lq_cabi::select_device(device);
		hipStream_t stream = nullptr;
		LQ_HIP_CHECK(hipStreamCreate(&stream));
		struct Closer { hipStream_t s; ~Closer() { (void)hipStreamDestroy(s); } } closer{stream};
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
	if (rc) g_reader_open_error = msg;                        // (lqreader_last_error(NULL))
	return rc;
}

int lqreader_inflate_stats(const lqreader *r, lqinflate_stats *stats)
{
	if (!r || !stats) return LQCOV_E_ARG;
	*stats = r->gzdev.stats;
	return 0;
}

int lqinflate_gzip(int device, const uint8_t *comp, uint64_t comp_len, uint32_t span_bytes, uint8_t *out, uint64_t out_cap, uint64_t *out_len,
                   lqinflate_stats *stats)
{
	char msg[512] = {0};
	const int rc = lq_cabi::guarded(msg, sizeof(msg), [&] {
		if (!out_len || (comp_len && !comp) || (out_cap && !out)) throw std::invalid_argument("null buffers");
		if (span_bytes && (span_bytes < 1024 || span_bytes > (1u << 17) || (span_bytes & 15))) throw std::invalid_argument("span_bytes must be a multiple of 16 from 1024 to 131072");
		*out_len = 0;
		lq_cabi::select_device(device);
		hipStream_t stream = nullptr;
		LQ_HIP_CHECK(hipStreamCreate(&stream));
		struct Closer { hipStream_t s; ~Closer() { (void)hipStreamDestroy(s); } } closer{stream};
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
		} catch (const GzipError &e) { throw std::runtime_error(std::string("failed to open file '(memory)': ") + e.what()); }
		*out_len = n;
		if (stats) *stats = g.stats;
	});
	if (rc) g_reader_open_error = msg;                        // (lqreader_last_error(NULL))
	return rc;
}

int lqinflate_blocks(int device, const uint8_t *comp, uint64_t comp_len, uint32_t n, const uint64_t *in_off, const uint32_t *in_len,
                     const uint64_t *out_off, const uint32_t *isize, uint8_t *out_host, uint32_t *status)
{
	char msg[512] = {0};
	const int rc = lq_cabi::guarded(msg, sizeof(msg), [&] {
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
		lq_cabi::select_device(device);
		hipStream_t stream = nullptr;
		LQ_HIP_CHECK(hipStreamCreate(&stream));
		struct Closer { hipStream_t s; ~Closer() { (void)hipStreamDestroy(s); } } closer{stream};
		InflateDev inf; DBuf out;
		out.ensure((size_t)out_len + 16);
		if (out_len) LQ_HIP_CHECK(hipMemcpyAsync(out.p, out_host, (size_t)out_len, hipMemcpyHostToDevice, stream));
		inf.run(stream, comp, comp_len, jobs, out.as<u8>(), status);
		if (out_len) LQ_HIP_CHECK(hipMemcpyAsync(out_host, out.p, (size_t)out_len, hipMemcpyDeviceToHost, stream));
		LQ_HIP_CHECK(hipStreamSynchronize(stream));
	});
	if (rc) g_reader_open_error = msg;                        // (lqreader_last_error(NULL))
	return rc;
}

int lqreader_names(const lqreader *r, const char **names, const uint64_t **name_off, const uint32_t **lens)
{
	if (!r || !names || !name_off || !lens) return LQCOV_E_ARG;
	*names = r->names.data(); *name_off = r->name_off.data(); *lens = r->lens.data();
	return 0;
}

} // extern "C"
