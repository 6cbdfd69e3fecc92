// longqc_amd/csrc/writer.cpp -- the FASTQ writer behind the C ABI of include/lqcov.h (lqchunk_fastq, lqfastq_*): the reads of a resident
// chunk (chunk.hpp), each cut to [begin, end), leave the device as the text `@name\nseq\n+\nqual\n` that lq_utils.write_fastq writes --
// sampleqc's --trim_output (longQC.py:345-346) and the FASTQ it converts a BAM file to (:302-303) -- without a read becoming an object
// on the host.  k_fastq_format (kernels_fastq.hpp) makes the text from the chunk's buffers; the host gives it three tables of one
// entry per read (where the record starts in the text, where its name starts, begin and end) and the record at every tile's start.
// lqchunk_fastq makes a whole chunk's text in one launch.  lqfastq_write streams it: the text is cut into pieces of piece_bytes (byte
// ranges, not records: a read of any length is nothing special), each piece is made on the device, copied into one of two page-locked
// buffers on the chunk's stream and handed to the writer thread, which appends it to the file while the next piece is made.
#include "chunk.hpp"
#include "kernels_fastq.hpp"
#include <algorithm>
#include <cerrno>
#include <condition_variable>
#include <fcntl.h>
#include <memory>
#include <mutex>
#include <thread>
#include <unistd.h>

// Pieces of 16 MiB: a piece's launch, copy and synchronisation cost some tens of microseconds, the copy itself (about 50 GB/s) 0.3 ms
// and the file write (a few GB/s into the page cache) several ms -- the fixed costs vanish, the writer thread is never short of
// bytes after the first piece, and the two page-locked buffers take 32 MiB whatever the chunk's size.
#define LQ_FASTQ_PIECE ((u64)16 << 20)

static_assert(LQ_FASTQ_PIECE % LQ_FASTQ_TILE == 0, "a piece is whole tiles");

namespace {
thread_local std::string g_fastq_error;                       // why lqfastq_open failed, and what lqfastq_close reported

template <class F> int fastq_guard(std::string &err, F &&f)
{
	try { f(); return 0; }
	catch (const lq_io_error &e) { err = e.what(); return LQCOV_E_IO; }
	catch (const std::domain_error &e) { err = e.what(); return LQCOV_E_DOMAIN; }
	catch (const std::invalid_argument &e) { err = e.what(); return LQCOV_E_ARG; }
	catch (const std::runtime_error &e) { err = e.what(); return LQCOV_E_DEVICE; }
	catch (const std::exception &e) { err = e.what(); return LQCOV_E_STATE; }
}

// the tables of k_fastq_format for the chunk's reads, on the device -> the bytes of the chunk's text
u64 fastq_tables(lqchunk &c, const char *names, const u64 *name_off, const u32 *begin, const u32 *end)
{
	if (!c.resident) throw std::logic_error("no chunk loaded (lqchunk_load)");
	if ((begin == nullptr) != (end == nullptr)) throw std::invalid_argument("begin and end come together");
	const u32 n = c.n;
	if (!n) return 0;                                         // (a chunk without reads: no text, whatever else it lacks)
	if (!c.has_qual) throw std::invalid_argument("the chunk holds no qualities");
	if (names && !name_off) throw std::invalid_argument("null buffers");
	std::vector<u64> rec((size_t)n + 1), noff(n, 0);
	std::vector<uint2> be(n);
	u64 blob0 = LQ_U64MAX, blob1 = 0;                              // the name bytes to upload: names[blob0 .. blob1)
	for (u32 i = 0; names && i < n; ++i) blob0 = std::min(blob0, name_off[i]);
	rec[0] = 0;
	for (u32 i = 0; i < n; ++i) {
		const u64 len = c.off[i + 1] - c.off[i];
		if (len > 0xffffffffULL) throw std::domain_error("a read of 2^32 bases or more");
		const u32 b = begin ? begin[i] : 0, e = end ? end[i] : (u32)len;
		if (b > e) throw std::invalid_argument("begin > end at read " + std::to_string(i));
		if (e > len) throw std::invalid_argument("end > the length of read " + std::to_string(i));
		u64 nl = 0;
		if (names) {
			nl = strlen(names + name_off[i]);
			noff[i] = name_off[i] - blob0;
			blob1 = std::max(blob1, name_off[i] + nl + 1);
		}
		be[i].x = b; be[i].y = e;
		rec[i + 1] = rec[i] + nl + 2 * (u64)(e - b) + 6;
	}
	const u64 total = rec[n], n_tiles = (total + LQ_FASTQ_TILE - 1) / LQ_FASTQ_TILE, blob = names ? blob1 - blob0 : 0;
	std::vector<u32> tile_rec((size_t)n_tiles + 1);               // the work list: the record that holds the first byte of every tile
	{
		u32 r = 0;
		for (u64 t = 0; t < n_tiles; ++t) {
			while (r + 1 < n && rec[r + 1] <= t * LQ_FASTQ_TILE) ++r;
			tile_rec[t] = r;
		}
		tile_rec[n_tiles] = n - 1;
	}
	lq_cabi::select_device(c.device);
	c.fq_names.ensure((size_t)blob + LQ_GATHER_SRC_PAD);           // (the funnel's second load: what it reads behind the blob is masked away)
	c.fq_noff.ensure((size_t)n * 8); c.fq_be.ensure((size_t)n * sizeof(uint2)); c.fq_rec.ensure(((size_t)n + 1) * 8); c.fq_tile.ensure((n_tiles + 1) * 4);
	if (blob) LQ_HIP_CHECK(hipMemcpyAsync(c.fq_names.p, names + blob0, (size_t)blob, hipMemcpyHostToDevice, c.stream));
	LQ_HIP_CHECK(hipMemcpyAsync(c.fq_noff.p, noff.data(), (size_t)n * 8, hipMemcpyHostToDevice, c.stream));
	LQ_HIP_CHECK(hipMemcpyAsync(c.fq_be.p, be.data(), (size_t)n * sizeof(uint2), hipMemcpyHostToDevice, c.stream));
	LQ_HIP_CHECK(hipMemcpyAsync(c.fq_rec.p, rec.data(), ((size_t)n + 1) * 8, hipMemcpyHostToDevice, c.stream));
	LQ_HIP_CHECK(hipMemcpyAsync(c.fq_tile.p, tile_rec.data(), (n_tiles + 1) * 4, hipMemcpyHostToDevice, c.stream));
	LQ_HIP_CHECK(hipStreamSynchronize(c.stream));             // (the host tables die here)
	return total;
}

// bytes [a, b) of the text (a: on a tile, b <= total) to dst, which holds them rounded up to whole 16-byte words
void fastq_launch(lqchunk &c, u64 total, u64 a, u64 b, u8 *dst)
{
	const u64 n_tiles = (b - a + LQ_FASTQ_TILE - 1) / LQ_FASTQ_TILE;
	const u32 grid = (u32)std::min<u64>(n_tiles, LQ_FASTQ_MAX_BLOCKS);
	LQ_LAUNCH(k_fastq_format, grid, LQ_FASTQ_THREADS, c.stream, c.seq.as<u8>(), c.qual.as<u8>(), c.d_off.as<u64>(), c.fq_names.as<u8>(), c.fq_noff.as<u64>(),
	          c.fq_be.as<uint2>(), c.fq_rec.as<u64>(), c.fq_tile.as<u32>(), a / LQ_FASTQ_TILE, n_tiles, total, dst);
	LQ_HIP_CHECK(hipGetLastError());
}
} // namespace

struct lqfastq {
	std::string path, err;
	int device = 0, rc = 0;                                   // rc: the first I/O or device error; every later call reports it again
	u64 piece = 0;
	int fd = -1;
	u8 *host[2] = {nullptr, nullptr};                         // page-locked, `piece` bytes each
	DBuf dev;                                                 // the piece as the kernel writes it
	hipEvent_t ev0 = nullptr, ev1 = nullptr;
	double kernel_ms = 0;
	// the hand-over: the caller fills slot next & 1 and sets its len, the thread writes the slots in turn and clears len.  stop: an
	// error on either side -- both waits look at it, so neither side waits for the other once it is set
	std::thread th;
	std::mutex mu;
	std::condition_variable cv;
	u64 len[2] = {0, 0}, next = 0;
	bool stop = false, done = false;
	std::string werr;                                         // the thread's error

	void thread_main()
	{
		for (u32 k = 0;; k ^= 1) {
			u64 n;
			{
				std::unique_lock<std::mutex> lk(mu);
				cv.wait(lk, [&] { return len[k] || stop || done; });
				if (stop || !len[k]) return;                  // (done: the slots are filled in turn, so nothing waits behind an empty one)
				n = len[k];
			}
			std::string e;
			for (u64 at = 0; at < n;) {
				const ssize_t w = ::write(fd, host[k] + at, (size_t)(n - at));
				if (w < 0 && errno == EINTR) continue;
				if (w <= 0) { e = "failed to write file '" + path + "': " + (w < 0 ? strerror(errno) : "no byte written"); break; }
				at += (u64)w;
			}
			std::lock_guard<std::mutex> lk(mu);
			if (!e.empty()) { werr = e; stop = true; cv.notify_all(); return; }
			len[k] = 0;
			cv.notify_all();
		}
	}

	void halt()                                               // the caller's side failed: the thread ends without writing what waits
	{
		{ std::lock_guard<std::mutex> lk(mu); stop = true; }
		cv.notify_all();
	}

	u64 write(lqchunk &c, const char *names, const u64 *name_off, const u32 *begin, const u32 *end)
	{
		if (c.device != device) throw std::invalid_argument("the chunk lives on another device than the writer");
		const u64 total = fastq_tables(c, names, name_off, begin, end);
		if (!total) return 0;                                  // (nothing to write: no file either, as write_fastq)
		if (fd < 0) {
			fd = ::open(path.c_str(), O_WRONLY | O_CREAT | O_APPEND | O_CLOEXEC, 0666);
			if (fd < 0) throw lq_open_error(path, strerror(errno));
			th = std::thread([this] { thread_main(); });
		}
		dev.ensure((size_t)piece);
		for (u64 a = 0; a < total; a += piece) {
			const u64 b = std::min(total, a + piece);
			const u32 k = (u32)(next & 1);
			{
				std::unique_lock<std::mutex> lk(mu);
				cv.wait(lk, [&] { return !len[k] || stop; });
				if (stop) throw lq_io_error(werr.empty() ? "the writer has stopped" : werr);
			}
			LQ_HIP_CHECK(hipEventRecord(ev0, c.stream));
			fastq_launch(c, total, a, b, dev.as<u8>());
			LQ_HIP_CHECK(hipEventRecord(ev1, c.stream));
			LQ_HIP_CHECK(hipMemcpyAsync(host[k], dev.p, (size_t)(b - a), hipMemcpyDeviceToHost, c.stream));
			LQ_HIP_CHECK(hipStreamSynchronize(c.stream));
			float ms = 0;
			LQ_HIP_CHECK(hipEventElapsedTime(&ms, ev0, ev1));
			kernel_ms += ms;
			{ std::lock_guard<std::mutex> lk(mu); len[k] = b - a; ++next; }
			cv.notify_all();
		}
		return total;
	}

	~lqfastq()
	{
		if (th.joinable()) { halt(); th.join(); }
		if (fd >= 0) ::close(fd);
		(void)hipSetDevice(device);
		for (u8 *p : host) if (p) (void)hipHostFree(p);
		if (ev0) (void)hipEventDestroy(ev0);
		if (ev1) (void)hipEventDestroy(ev1);
	}
};

extern "C" {

int lqchunk_fastq(lqchunk *c, const char *names, const uint64_t *name_off, const uint32_t *begin, const uint32_t *end, uint8_t *out, uint64_t out_cap,
                  uint64_t *out_len)
{
	if (!c) return LQCOV_E_ARG;
	return fastq_guard(c->err, [&] {
		if (!out_len) throw std::invalid_argument("null buffers");
		const u64 total = fastq_tables(*c, names, name_off, begin, end);
		*out_len = total;
		if (total > out_cap) throw std::invalid_argument("out_cap is smaller than the text");
		if (!total) return;
		if (!out) throw std::invalid_argument("null buffers");
		c->fq_text.ensure((size_t)((total + 15) / 16 * 16));
		fastq_launch(*c, total, 0, total, c->fq_text.as<u8>());
		LQ_HIP_CHECK(hipMemcpyAsync(out, c->fq_text.p, (size_t)total, hipMemcpyDeviceToHost, c->stream));
		LQ_HIP_CHECK(hipStreamSynchronize(c->stream));
	});
}

lqfastq *lqfastq_open(const char *path, int device, uint64_t piece_bytes)
{
	std::unique_ptr<lqfastq> w;
	const int rc = fastq_guard(g_fastq_error, [&] {
		if (!path || !*path) throw std::invalid_argument("no path");
		if (piece_bytes % LQ_FASTQ_TILE) throw std::invalid_argument("piece_bytes must be a multiple of " + std::to_string(LQ_FASTQ_TILE));
		lq_cabi::select_device(device);
		w.reset(new lqfastq());
		w->path = path; w->device = device; w->piece = piece_bytes ? piece_bytes : LQ_FASTQ_PIECE;
		for (u8 *&p : w->host) LQ_HIP_CHECK(hipHostMalloc((void**)&p, (size_t)w->piece));
		LQ_HIP_CHECK(hipEventCreate(&w->ev0));
		LQ_HIP_CHECK(hipEventCreate(&w->ev1));
	});
	return rc ? nullptr : w.release();
}

int lqfastq_write(lqfastq *w, lqchunk *c, const char *names, const uint64_t *name_off, const uint32_t *begin, const uint32_t *end, uint64_t *bytes_written)
{
	if (!w) return LQCOV_E_ARG;
	if (!c) { w->err = "no chunk"; return LQCOV_E_ARG; }
	if (w->rc) return w->rc;                                  // (w->err still says why)
	std::string err;
	const int rc = fastq_guard(err, [&] {
		const u64 n = w->write(*c, names, name_off, begin, end);
		if (bytes_written) *bytes_written = n;
	});
	if (rc) {
		w->err = err;
		if (rc != LQCOV_E_ARG && rc != LQCOV_E_DOMAIN && rc != LQCOV_E_STATE) { w->rc = rc; w->halt(); }      // (a refused argument wrote nothing: the writer stays usable)
	}
	return rc;
}

int lqfastq_close(lqfastq *w)
{
	if (!w) return LQCOV_E_ARG;
	{ std::lock_guard<std::mutex> lk(w->mu); w->done = true; }
	w->cv.notify_all();
	if (w->th.joinable()) w->th.join();                       // (it has written every piece handed over, or stopped at an error)
	int rc = w->rc;
	if (!rc && !w->werr.empty()) { rc = LQCOV_E_IO; w->err = w->werr; }
	if (w->fd >= 0) {
		const int e = ::close(w->fd);
		w->fd = -1;
		if (e != 0 && !rc) { rc = LQCOV_E_IO; w->err = "failed to close file '" + w->path + "': " + strerror(errno); }
	}
	g_fastq_error = rc ? w->err : std::string();
	delete w;
	return rc;
}

const char *lqfastq_last_error(const lqfastq *w) { return w ? w->err.c_str() : g_fastq_error.c_str(); }

double lqfastq_kernel_ms(const lqfastq *w) { return w ? w->kernel_ms : 0.0; }

} // extern "C"
