// longqc_amd/csrc/bgzf.hpp -- BGZF, the container of BAM (SAM specification 4.1): a sequence of gzip members of at most 64 KiB, each
// with an extra subfield 'B','C' that holds the member's size minus one (BSIZE) and, as every gzip member, the CRC32 and the size of
// its inflated bytes (ISIZE) in its last eight bytes.  The members are independent deflate streams, so the sizes alone say where
// each one's bytes land and a pool of threads inflates them side by side, straight into the caller's buffer.  A unit of its own: it
// knows nothing of what the bytes are (reader.cpp's BAM branch; a bgzip-compressed FASTA/FASTQ goes through gzread unless the reader
// is in device mode).  The second way, opt-in: `device` set, the listed blocks are inflated by k_bgzf_inflate (kernels_inflate.hpp) --
// the owner's hook uploads the compressed bytes, launches and brings the inflated bytes back to dst and one status per block -- and
// the pool only checks the CRC32 of what came back, which vouches for the kernel and for the copy alike.  The errors are the same
// three, for the same blocks.  Where the hook leaves the bytes on the device (reader.cpp, lqreader_host_copy) it fills dev_crc with
// the blocks' CRC32 as the device computed them, and those are compared instead.
#pragma once
#include "lq_cabi.hpp"
#include <zlib.h>
#include <fcntl.h>
#include <unistd.h>
#include <atomic>
#include <functional>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

struct BgzfInflater {
	static constexpr u64 WINDOW = (u64)8 << 20, MAX_BLOCK = 65536;
	int fd = -1;                                              // not owned
	int n_threads = 1;
	u64 next = 0;                                             // the file offset of the next block
	bool ended = false;                                       // the file's last block has been inflated
	std::vector<u8> win; u64 win_at = 0, win_len = 0; bool win_eof = false;      // compressed bytes win_at .. win_at + win_len of the file

	struct Block { u64 at, in, in_len, isize, out; u32 crc; };        // at: file offset; in: deflate bytes in win; out: offset in the caller's buffer
	// device mode: inflate `blocks` (their bytes: win) into dst[0 .. out_bytes) -> status[i]: 0 fine, 1 not a deflate stream, other: the
	// stream does not give isize bytes (LQ_INF_* of kernels_inflate.hpp)
	std::function<void(const std::vector<Block> &blocks, const u8 *win, u8 *dst, u64 out_bytes, std::vector<u32> &status)> device;
	std::vector<u32> dev_crc;                                 // `device` may fill it, one CRC32 per block: dst then holds nothing

	[[noreturn]] static void fail(u64 at, const char *what)
	{
		throw lq_file_error("BGZF block at file offset " + std::to_string(at) + ": " + what);
	}

	static u32 le32(const u8 *p) { return (u32)p[0] | (u32)p[1] << 8 | (u32)p[2] << 16 | (u32)p[3] << 24; }

	// the size of the block whose header is at p (n bytes there), 0: no BGZF header; *hdr: the bytes in front of the deflate stream
	static u64 block_size(const u8 *p, u64 n, u64 *hdr)
	{
		if (n < 18 || p[0] != 0x1f || p[1] != 0x8b || p[2] != 8 || !(p[3] & 4)) return 0;
		const u64 xlen = (u64)p[10] | (u64)p[11] << 8;
		if (12 + xlen > n) return 0;
		for (u64 q = 12; q + 4 <= 12 + xlen;) {
			const u64 slen = (u64)p[q + 2] | (u64)p[q + 3] << 8;
			if (p[q] == 'B' && p[q + 1] == 'C' && slen == 2 && q + 6 <= 12 + xlen) {
				*hdr = 12 + xlen;
				const u64 size = ((u64)p[q + 4] | (u64)p[q + 5] << 8) + 1;
				return size >= *hdr + 8 ? size : 0;
			}
			q += 4 + slen;
		}
		return 0;
	}

	// the window holds the file from `next` on: at least one whole block, or all that is left of the file
	void slide()
	{
		if (win.empty()) win.resize(WINDOW);
		if (next >= win_at && next + MAX_BLOCK <= win_at + win_len) return;
		if (win_eof && next >= win_at) return;
		u64 keep = 0;
		if (next >= win_at && next < win_at + win_len) {
			keep = win_at + win_len - next;
			memmove(win.data(), win.data() + (next - win_at), (size_t)keep);
		}
		win_at = next; win_len = keep; win_eof = false;
		while (win_len < WINDOW) {
			const ssize_t got = ::pread(fd, win.data() + win_len, (size_t)(WINDOW - win_len), (off_t)(win_at + win_len));
			if (got < 0) throw lq_file_error("read error");
			if (got == 0) { win_eof = true; break; }
			win_len += (u64)got;
		}
	}

	// whole blocks into dst[0 .. room): -> the bytes made.  0 with ended: the file is over; 0 without: the next block needs *need bytes.
	// max_blocks: stop behind that many blocks (0: as many as there is room for)
	u64 fill(u8 *dst, u64 room, u64 *need, u64 max_blocks = 0)
	{
		std::vector<Block> blocks;
		u64 out = 0;
		*need = 0;
		while (!ended && out == 0) {
			slide();
			blocks.clear();
			for (;;) {
				const u64 o = next - win_at, left = win_len - o;
				if (left == 0 && win_eof) { ended = true; break; }
				u64 hdr = 0;
				const u64 size = block_size(win.data() + o, left, &hdr);
				if (!size) {
					if (left < 18 && !win_eof) break;
					fail(next, left < 18 ? "cut short by the end of the file" : "not a BGZF block header");
				}
				if (size > left) {
					if (win_eof) fail(next, "cut short by the end of the file");
					break;
				}
				const u8 *b = win.data() + o;
				const u64 isize = le32(b + size - 4);
				if (isize > MAX_BLOCK) fail(next, "ISIZE above 65536");
				if (out + isize > room) { if (blocks.empty()) *need = isize; break; }
				if (max_blocks && blocks.size() == max_blocks) break;
				blocks.push_back({next, o + hdr, size - hdr - 8, isize, out, le32(b + size - 8)});
				out += isize; next += size;
			}
			if (blocks.empty()) break;
			inflate_all(blocks, dst, out);
		}
		return out;
	}

	void inflate_all(const std::vector<Block> &blocks, u8 *dst, u64 out_bytes)
	{
		std::vector<u32> status;
		dev_crc.clear();
		if (device) device(blocks, win.data(), dst, out_bytes, status);
		const bool crc_known = dev_crc.size() == blocks.size() && !blocks.empty();
		const u32 nt = (u32)std::min<u64>((u64)std::max(n_threads, 1), blocks.size());
		std::atomic<u64> turn{0};
		std::vector<u64> bad_at(nt, LQ_U64MAX); std::vector<const char*> bad(nt, nullptr);
		auto work = [&](u32 w) {
			if (device) {                                             // the bytes are there: what the kernel said of them, then the CRC32
				for (u64 i; (i = turn.fetch_add(1)) < blocks.size();) {
					const Block &b = blocks[i];
					const char *what = nullptr;
					if (status[i]) what = status[i] == 1 ? "corrupt deflate stream" : "ISIZE does not match the inflated bytes";
					else if ((crc_known ? dev_crc[i] : (u32)crc32(crc32(0L, Z_NULL, 0), dst + b.out, (uInt)b.isize)) != b.crc) what = "CRC32 mismatch";
					if (what && b.at < bad_at[w]) { bad_at[w] = b.at; bad[w] = what; }
				}
				return;
			}
			z_stream z; memset(&z, 0, sizeof(z));
			if (inflateInit2(&z, -15) != Z_OK) { bad_at[w] = 0; bad[w] = "no memory for zlib"; return; }
			for (u64 i; (i = turn.fetch_add(1)) < blocks.size();) {
				const Block &b = blocks[i];
				u8 none[1];
				inflateReset(&z);
				z.next_in = win.data() + b.in; z.avail_in = (uInt)b.in_len;
				z.next_out = b.isize ? dst + b.out : none; z.avail_out = b.isize ? (uInt)b.isize : 1;
				const int rc = inflate(&z, Z_FINISH);
				const char *what = nullptr;
				if (rc != Z_STREAM_END || z.total_out != b.isize) what = rc == Z_STREAM_END || rc == Z_BUF_ERROR || rc == Z_OK ? "ISIZE does not match the inflated bytes" : "corrupt deflate stream";
				else if ((u32)crc32(crc32(0L, Z_NULL, 0), b.isize ? dst + b.out : none, (uInt)b.isize) != b.crc) what = "CRC32 mismatch";
				if (what && b.at < bad_at[w]) { bad_at[w] = b.at; bad[w] = what; }
			}
			inflateEnd(&z);
		};
		if (nt <= 1) work(0);
		else {
			std::vector<std::thread> pool;
			for (u32 w = 1; w < nt; ++w) pool.emplace_back(work, w);
			work(0);
			for (auto &t : pool) t.join();
		}
		u32 first = nt;
		for (u32 w = 0; w < nt; ++w) if (bad[w] && (first == nt || bad_at[w] < bad_at[first])) first = w;
		if (first != nt) fail(bad_at[first], bad[first]);
	}
};
