// longqc_amd/csrc/gzip.hpp -- a gzip file that is not BGZF (RFC 1952: members of header, deflate stream, CRC32, ISIZE), inflated on
// the device by speculative spans (kernels_gzip.hpp).  The second way to read such a file, opt-in (reader.cpp, lqreader_inflate);
// what it hands out is what gzread hands out for the same file, byte for byte, and where gzread fails it fails.
//
// The host walks the members: it parses the header (FEXTRA, FNAME, FCOMMENT, FHCRC) and the trailer, and behind a member follows
// gzread -- two bytes of magic begin another member, anything else is ignored, and a file that ends inside a header, a block or a
// trailer just ends (zlib's Z_BUF_ERROR, which gzread does not report); a bad method, reserved flags, a header CRC, a corrupt block, a
// wrong CRC32 or ISIZE are "not a complete gzip stream".  The deflate stream between them is the device's, a launch at a time:
//   * a window of the compressed bytes goes up, from the block boundary the stream has reached (bit `pos_bit` of the file);
//   * k_gz_find, k_gz_inflate_spec: span 0 starts at that boundary, the others where the search found a header;
//   * the chain: span i + 1 is accepted only if it starts at the bit where accepted span i ended.  The first break ends what the
//     launch contributes -- a false positive of the search, an empty span, a block the search does not look for, a region that
//     was too small, the member's end, the room the caller has: all the same rule -- and the next launch starts at the last
//     accepted end;
//   * k_gz_window, k_gz_resolve put the accepted spans' bytes where the caller's device buffer wants them; they come back for the
//     record parser and for the CRC32, which vouches for kernels and copies alike; the last window stays on the device.
// What the device cannot vouch for goes to zlib, one block at a time from the last accepted boundary (raw inflate, inflatePrime for
// the bit offset, inflateSetDictionary for the window): a span that reports an error, a marker in front of the member's first byte,
// a block that does not fit a span's region even after the region was doubled once.  zlib's verdict decides, and its bytes go on
// as if the device had made them.
// keep_on_device (reader.cpp, lqreader_host_copy): the accepted bytes do not come back.  Their CRC32 is k_crc32_ranges' over the
// caller's device buffer, folded into the member's by length; the member's last 32 KiB then exist only as the device's window behind
// the last accepted span (d_wins), and come to hwin when zlib needs them as its dictionary.
#pragma once
#include "lq_cabi.hpp"
#include "kernels_gzip.hpp"
#include "kernels_crc32.hpp"
#include <zlib.h>
#include <unistd.h>
#include <functional>

struct GzipError : lq_file_error { GzipError() : lq_file_error("not a complete gzip stream") {} };

struct GzipInflater {
	// the input: a descriptor (not owned) or bytes in memory
	int fd = -1; const u8 *mem = nullptr; u64 mem_len = 0;
	u32 span_bytes = 16384;
	hipStream_t stream = nullptr;
	// where the device wants the n bytes that go to dst on the host (the owner makes room and keeps what is in front of them)
	std::function<u8*(u8 *dst, u64 n)> dev_room;
	lqinflate_stats stats{};
	bool done = false;                                        // nothing more comes
	bool keep_on_device = false;                              // what a launch accepts is not copied to dst
	lqcopy_stats *copied = nullptr;                           // the owner's account of what moved and who made the CRC32
	CrcDev crcdev;
	bool hwin_dev = false;                                    // hwin is stale: the window is d_wins[win_slot]

	enum { HEADER = 0, BODY, ZBLOCK, TRAILER };
	int state = HEADER;
	u64 at = 0;                                               // HEADER, TRAILER: the file offset
	u64 pos_bit = 0;                                          // BODY, ZBLOCK: the block boundary reached, a bit offset of the file
	bool first_member = true, doubled = false, failed = false;
	std::vector<u8> hwin;                                     // the member's last bytes, at most 32 KiB
	u32 crc = 0; u64 isize = 0;
	u64 min_spans = 0;                                        // a block ran past the last window: the next one has at least this many spans
	double ratio = 4.0;                                       // inflated bytes per compressed byte, as the last launch saw it
	z_stream z; bool z_open = false, z_active = false; u64 z_next = 0, z_first = 0; std::vector<u8> z_in;
	std::vector<u8> cwin; u64 cw_at = 0, cw_len = 0; bool cw_eof = false;
	DBuf d_comp, d_start, d_jobs, d_spans, d_syms, d_acc, d_wins, d_status, d_markers;
	u64 win_slot = 0; bool dwin_ok = false;                   // the window behind the last launch is wins[win_slot]

	~GzipInflater() { if (z_open) inflateEnd(&z); }

	static u32 span_bytes_env()
	{
		const char *e = getenv("LQREADER_GZ_SPAN_BYTES");
		const u64 v = e ? strtoull(e, nullptr, 10) : 0;
		return v ? (u32)std::min<u64>(std::max<u64>(v, 1024), (u64)1 << 17) & ~15u : 16384u;
	}

	// up to n bytes of the file from offset off -> how many there are
	u64 fetch(u64 off, u8 *dst, u64 n)
	{
		if (mem) {
			if (off >= mem_len) return 0;
			n = std::min(n, mem_len - off);
			memcpy(dst, mem + off, (size_t)n);
			return n;
		}
		u64 have = 0;
		while (have < n) {
			const ssize_t got = ::pread(fd, dst + have, (size_t)(n - have), (off_t)(off + have));
			if (got < 0) throw lq_file_error("read error");
			if (got == 0) break;
			have += (u64)got;
		}
		return have;
	}

	// cwin holds the file's bytes [off, off + n), or what there is of them: -> how many
	u64 window(u64 off, u64 n)
	{
		if (cwin.size() < n + LQ_INFLATE_PAD) cwin.resize((size_t)n + LQ_INFLATE_PAD);
		cw_at = off;
		cw_len = fetch(off, cwin.data(), n);
		cw_eof = cw_len < n;
		return cw_len;
	}

	u64 hist() const { return std::min<u64>(isize, LQ_GZ_WIN); }      // hwin's size, where hwin is on the host

	void fetch_hwin()                                         // the window comes to the host
	{
		const u64 h = hist();
		hwin.resize((size_t)h);
		if (h) {
			LQ_HIP_CHECK(hipMemcpyAsync(hwin.data(), d_wins.as<u8>() + win_slot * LQ_GZ_WIN + (LQ_GZ_WIN - h), (size_t)h, hipMemcpyDeviceToHost, stream));
			LQ_HIP_CHECK(hipStreamSynchronize(stream));
		}
		hwin_dev = false;
	}

	void made_on_device(const u8 *d_p, u64 n)                 // n bytes of the member have come out and lie at d_p on the device
	{
		const u64 zero = 0; u32 c = 0;
		crcdev.run(stream, d_p, 1, &zero, &n, &c);
		crc = (u32)crc32_combine(crc, c, (z_off_t)n);
		isize += n;
		hwin_dev = true;
		if (copied) copied->bytes_crc_device += n;
	}

	void made(const u8 *p, u64 n)                             // n bytes of the member have come out
	{
		if (copied) copied->bytes_crc_host += n;
		for (u64 o = 0; o < n; o += 1u << 30) crc = (u32)crc32(crc, p + o, (uInt)std::min<u64>(n - o, 1u << 30));
		isize += n;
		if (n >= LQ_GZ_WIN) hwin.assign(p + n - LQ_GZ_WIN, p + n);
		else {
			if (hwin.size() + n > LQ_GZ_WIN) hwin.erase(hwin.begin(), hwin.begin() + (size_t)(hwin.size() + n - LQ_GZ_WIN));
			hwin.insert(hwin.end(), p, p + n);
		}
	}

	// bytes into dst[0 .. room) -> how many.  0 with done: the stream is over; 0 without: *need says how much room the next bytes want
	u64 fill(u8 *dst, u64 room, u64 *need)
	{
		*need = 0;
		if (failed) throw GzipError();
		while (!done) {
			u64 out = 0;
			try {
				switch (state) {
				case HEADER: header(); break;
				case TRAILER: trailer(); break;
				case BODY: out = launch(dst, room, need); break;
				default: out = zblock(dst, room); break;
				}
			} catch (const GzipError &) { failed = true; throw; }
			if (out || *need) return out;
			if (!room) { *need = 1; return 0; }
		}
		return 0;
	}

	// RFC 1952 2.3; gzread: less than two bytes or no magic behind a member is the end, a header the file ends in as well
	void header()
	{
		u64 n = 1 << 16;
		for (;;) {
			const u64 have = window(at, n);
			const u8 *p = cwin.data();
			if (have < 2 || p[0] != 0x1f || p[1] != 0x8b) {
				if (first_member && have >= 2) throw GzipError();
				done = true; return;
			}
			bool more = false;
			auto want = [&](u64 upto) { if (upto > have) { more = true; return false; } return true; };
			u64 q = 10;
			do {
				if (!want(10)) break;
				if (p[2] != 8 || (p[3] & 0xe0)) throw GzipError();
				const u32 flg = p[3];
				if (flg & 4) { if (!want(q + 2)) break; q += 2 + ((u64)p[q] | (u64)p[q + 1] << 8); if (!want(q)) break; }
				for (int f = 8; f <= 16 && !more; f <<= 1) if (flg & f) {
					const u8 *e = q < have ? (const u8*)memchr(p + q, 0, (size_t)(have - q)) : nullptr;
					if (!e) { more = true; break; }
					q = (u64)(e - p) + 1;
				}
				if (more) break;
				if (flg & 2) {
					if (!want(q + 2)) break;
					if (((u32)crc32(crc32(0L, Z_NULL, 0), p, (uInt)q) & 0xffff) != ((u32)p[q] | (u32)p[q + 1] << 8)) throw GzipError();
					q += 2;
				}
			} while (0);
			if (more) {
				if (cw_eof) { done = true; return; }                  // the file ends inside the header
				n *= 2;
				continue;
			}
			first_member = false;
			pos_bit = (at + q) * 8; hwin.clear(); hwin_dev = false; crc = (u32)crc32(0L, Z_NULL, 0); isize = 0; dwin_ok = false; doubled = false;
			state = BODY;
			return;
		}
	}

	void trailer()
	{
		const u64 have = window(at, 8);
		if (have < 8) { done = true; return; }                    // the file ends inside the trailer
		const u8 *p = cwin.data();
		const u32 c = (u32)p[0] | (u32)p[1] << 8 | (u32)p[2] << 16 | (u32)p[3] << 24, n = (u32)p[4] | (u32)p[5] << 8 | (u32)p[6] << 16 | (u32)p[7] << 24;
		if (c != crc || n != (u32)isize) throw GzipError();
		at += 8;
		state = HEADER;
	}

	void block_end(bool final)                                // pos_bit is a block boundary: behind a final block the trailer begins at the next byte
	{
		if (final) { at = (pos_bit + 7) / 8; state = TRAILER; }
		else state = BODY;
	}

	u32 region() const { return std::max<u32>(span_bytes * 16, 128u << 10) * (doubled ? 2 : 1); }      // symbols of one span

	// one launch from pos_bit on
	u64 launch(u8 *dst, u64 room, u64 *need)
	{
		const u64 base = (pos_bit / 8) & ~(u64)15;
		const u32 first_bit = (u32)(pos_bit - base * 8);
		u64 want_spans = (u64)((double)room / (ratio * 1.05 * span_bytes)) + 1;
		want_spans = std::min<u64>(std::max<u64>(want_spans, min_spans), LQ_GZ_MAX_SPANS);
		const u64 len = window(base, want_spans * span_bytes);
		if (len * 8 <= first_bit) { state = ZBLOCK; return 0; }    // (nothing is left: zlib says what that is)
		const u32 n_spans = (u32)((len + span_bytes - 1) / span_bytes);
		++stats.launches;
		d_comp.ensure((size_t)(len + 3) / 4 * 4 + LQ_INFLATE_PAD);
		LQ_HIP_CHECK(hipMemcpyAsync(d_comp.p, cwin.data(), (size_t)len, hipMemcpyHostToDevice, stream));
		std::vector<u32> start(n_spans, LQ_GZ_NONE);
		if (n_spans > 1) {
			d_start.ensure((size_t)n_spans * 4);
			LQ_LAUNCH(k_gz_find, std::min<u32>(n_spans - 1, LQ_GZ_MAX_BLOCKS), LQ_GZ_THREADS, stream, d_comp.as<u8>(), (u32)len, span_bytes, n_spans, d_start.as<u32>());
			LQ_HIP_CHECK(hipGetLastError());
			LQ_HIP_CHECK(hipMemcpyAsync(start.data() + 1, d_start.as<u32>() + 1, (size_t)(n_spans - 1) * 4, hipMemcpyDeviceToHost, stream));
			LQ_HIP_CHECK(hipStreamSynchronize(stream));
		}
		start[0] = first_bit;
		// the jobs: the non-empty spans, each up to the next one's start
		const u32 reg = region();
		std::vector<GzJob> jobs;
		for (u32 s = 0; s < n_spans; ++s) if (start[s] != LQ_GZ_NONE && (s == 0 || start[s] > first_bit)) {
			if (!jobs.empty()) jobs.back().stop_bit = start[s];
			jobs.push_back({(u64)jobs.size() * reg, start[s], LQ_GZ_NONE, reg, s == 0 ? (u32)hist() : LQ_GZ_NONE});
		}
		const u32 nj = (u32)jobs.size();
		stats.spans_found += nj - 1;
		jobs[0].cap = (u32)std::min<u64>(reg, (room + 7) & ~(u64)7);
		d_jobs.ensure((size_t)nj * sizeof(GzJob)); d_spans.ensure((size_t)nj * sizeof(GzSpan)); d_syms.ensure((size_t)nj * reg * 2);
		LQ_HIP_CHECK(hipMemcpyAsync(d_jobs.p, jobs.data(), (size_t)nj * sizeof(GzJob), hipMemcpyHostToDevice, stream));
		LQ_LAUNCH(k_gz_inflate_spec, std::min<u32>(nj, LQ_GZ_MAX_BLOCKS), LQ_GZ_THREADS, stream, d_comp.as<u8>(), (u32)len, d_jobs.as<GzJob>(), nj, d_syms.as<u16>(), d_spans.as<GzSpan>());
		LQ_HIP_CHECK(hipGetLastError());
		std::vector<GzSpan> spans(nj);
		LQ_HIP_CHECK(hipMemcpyAsync(spans.data(), d_spans.p, (size_t)nj * sizeof(GzSpan), hipMemcpyDeviceToHost, stream));
		LQ_HIP_CHECK(hipStreamSynchronize(stream));
		// the chain
		std::vector<GzAcc> acc;
		u32 expect = first_bit, why = LQ_GZ_OK; u64 cum = 0; bool final = false, no_room = false, short_window = false;
		for (u32 j = 0; j < nj; ++j) {
			GzSpan &r = spans[j];
			if (r.start_bit != expect) break;
			if (r.status == LQ_GZ_INPUT && !cw_eof) { r.status = LQ_GZ_OK; short_window = r.end_bit == r.start_bit; }      // the window's end, not the file's
			if (r.end_bit == r.start_bit) { why = r.status; break; }       // not one whole block
			if (cum + r.n_out > room) { no_room = true; if (acc.empty()) *need = r.n_out; break; }
			acc.push_back({jobs[j].sym_off, cum, r.n_out, (u32)std::min<u64>(hist() + cum, LQ_GZ_WIN)});
			cum += r.n_out; expect = r.end_bit;
			if (r.saw_final) { final = true; break; }
			if (r.status != LQ_GZ_OK) { why = r.status; break; }
		}
		u32 n_acc = (u32)acc.size();
		u8 *d_out = nullptr;
		if (n_acc) {
			d_out = dev_room(dst, cum);
			if (hwin_dev && !dwin_ok) fetch_hwin();
			d_acc.ensure((size_t)n_acc * sizeof(GzAcc)); d_status.ensure((size_t)n_acc * 4); d_markers.ensure(8);
			const u64 slots = (u64)n_acc + 1;
			if (d_wins.cap < slots * LQ_GZ_WIN) {                     // (the window of the launch before moves with it)
				DBuf nb; nb.ensure((size_t)(slots * LQ_GZ_WIN));
				if (dwin_ok) LQ_HIP_CHECK(hipMemcpyAsync(nb.p, d_wins.as<u8>() + win_slot * LQ_GZ_WIN, LQ_GZ_WIN, hipMemcpyDeviceToDevice, stream));
				LQ_HIP_CHECK(hipStreamSynchronize(stream));
				d_wins.swap(nb); nb.release();
			} else if (dwin_ok && win_slot) LQ_HIP_CHECK(hipMemcpyAsync(d_wins.p, d_wins.as<u8>() + win_slot * LQ_GZ_WIN, LQ_GZ_WIN, hipMemcpyDeviceToDevice, stream));
			if (!dwin_ok && !hwin.empty())
				LQ_HIP_CHECK(hipMemcpyAsync(d_wins.as<u8>() + (LQ_GZ_WIN - hwin.size()), hwin.data(), hwin.size(), hipMemcpyHostToDevice, stream));
			LQ_HIP_CHECK(hipMemcpyAsync(d_acc.p, acc.data(), (size_t)n_acc * sizeof(GzAcc), hipMemcpyHostToDevice, stream));
			LQ_HIP_CHECK(hipMemsetAsync(d_status.p, 0, (size_t)n_acc * 4, stream));
			LQ_HIP_CHECK(hipMemsetAsync(d_markers.p, 0, 8, stream));
			LQ_LAUNCH(k_gz_window, 1, LQ_GZ_WINDOW_THREADS, stream, d_syms.as<u16>(), d_acc.as<GzAcc>(), n_acc, d_wins.as<u8>(), d_status.as<u32>());
			LQ_LAUNCH(k_gz_resolve, std::min<u32>(n_acc, LQ_GZ_MAX_BLOCKS), LQ_GZ_RESOLVE_THREADS, stream, d_syms.as<u16>(), d_acc.as<GzAcc>(), n_acc, d_wins.as<u8>(), d_out,
			          d_status.as<u32>(), (unsigned long long*)d_markers.p);
			LQ_HIP_CHECK(hipGetLastError());
			std::vector<u32> status(n_acc); unsigned long long markers = 0;
			LQ_HIP_CHECK(hipMemcpyAsync(status.data(), d_status.p, (size_t)n_acc * 4, hipMemcpyDeviceToHost, stream));
			LQ_HIP_CHECK(hipMemcpyAsync(&markers, d_markers.p, 8, hipMemcpyDeviceToHost, stream));
			if (cum && !keep_on_device) LQ_HIP_CHECK(hipMemcpyAsync(dst, d_out, (size_t)cum, hipMemcpyDeviceToHost, stream));
			LQ_HIP_CHECK(hipStreamSynchronize(stream));
			stats.markers_resolved += markers;
			for (u32 k = 0; k < n_acc; ++k) if (status[k]) {          // a marker in front of the member: zlib's from that span on
				n_acc = k; cum = acc[k].out_off; expect = k ? spans[k - 1].end_bit : first_bit;
				final = false; no_room = false; why = LQ_GZ_INVALID;
				break;
			}
			// (the window behind the last span that counts is whole whatever a later span's markers pointed at: where the bytes stay on
			// the device it is the only copy of the member's last bytes)
			dwin_ok = keep_on_device || n_acc == acc.size(); win_slot = n_acc;
		}
		if (n_acc) {
			if (keep_on_device) made_on_device(d_out, cum);
			else { made(dst, cum); if (copied) copied->bytes_to_host += cum; }
			stats.spans_accepted += n_acc - 1; stats.bytes_device += cum;
			const u64 in_bits = expect - first_bit;
			if (in_bits >= 8 * (u64)span_bytes) ratio = std::min(std::max((double)cum * 8 / (double)in_bits, 1.0), 1000.0);
			doubled = false; min_spans = 0;
		} else if (short_window) {
			if (n_spans >= LQ_GZ_MAX_SPANS) why = LQ_GZ_INPUT;        // (a block longer than the longest window: zlib's)
			else min_spans = 2 * (u64)n_spans;
		}
		stats.spans_rejected += nj - std::max<u32>(n_acc, 1);
		pos_bit = base * 8 + expect;
		if (final) block_end(true);
		else if (why == LQ_GZ_INVALID || why == LQ_GZ_INPUT) state = ZBLOCK;
		else if (why == LQ_GZ_FULL && !n_acc) {
			if (jobs[0].cap < reg) *need = (u64)reg;              // (it was the caller's room that was full)
			else if (!doubled) doubled = true;
			else state = ZBLOCK;
		}
		if (n_acc) *need = 0;
		(void)no_room;
		return cum;
	}

	// zlib from pos_bit to the end of that block, as much of it as the room takes
	u64 zblock(u8 *dst, u64 room)
	{
		if (!z_active) {
			if (!z_open) {
				memset(&z, 0, sizeof(z));
				if (inflateInit2(&z, -15) != Z_OK) throw std::runtime_error("no memory for zlib");
				z_open = true;
			} else inflateReset2(&z, -15);
			z_next = pos_bit / 8; z.avail_in = 0;
			const u32 r = (u32)(pos_bit & 7);
			if (r) {
				u8 byte = 0;
				if (fetch(z_next, &byte, 1) == 1) { inflatePrime(&z, 8 - (int)r, byte >> r); ++z_next; }
			}
			z_first = z_next;
			if (hwin_dev) fetch_hwin();
			if (!hwin.empty()) inflateSetDictionary(&z, hwin.data(), (uInt)hwin.size());
			z_active = true;
			z_in.resize(1 << 16);
		}
		z.next_out = dst; z.avail_out = (uInt)std::min<u64>(room, 1u << 30);
		const uLong out0 = z.total_out;
		bool ended = false, final = false, cut = false;
		while (z.avail_out) {
			if (z.avail_in == 0) {
				const u64 got = fetch(z_next, z_in.data(), z_in.size());
				z.next_in = z_in.data(); z.avail_in = (uInt)got; z_next += got;
			}
			const bool eof = z.avail_in == 0;
			const uLong in0 = z.total_in; const uInt av0 = z.avail_out;
			const int rc = inflate(&z, Z_BLOCK);
			if (rc == Z_DATA_ERROR || rc == Z_NEED_DICT || rc == Z_MEM_ERROR || rc == Z_STREAM_ERROR) { ended = true; failed = true; break; }
			if (rc == Z_STREAM_END || (z.data_type & 128)) { ended = true; final = rc == Z_STREAM_END || (z.data_type & 64); break; }
			if (eof && z.total_in == in0 && z.avail_out == av0) { ended = true; cut = true; break; }      // the file ends inside the block
		}
		const u64 out = (u64)(z.total_out - out0);
		if (out) {
			u8 *d = dev_room(dst, out);
			LQ_HIP_CHECK(hipMemcpyAsync(d, dst, (size_t)out, hipMemcpyHostToDevice, stream));
			LQ_HIP_CHECK(hipStreamSynchronize(stream));
			made(dst, out);
			stats.bytes_zlib += out;
			dwin_ok = false;
		}
		if (ended) {
			z_active = false; doubled = false;
			if (failed) throw GzipError();                        // (as gzread: the bytes of the call that fails are not handed out)
			else if (cut) done = true;
			else {
				pos_bit = (z_first + z.total_in) * 8 - (u64)(z.data_type & 63);
				block_end(final);
			}
		}
		return out;
	}
};
