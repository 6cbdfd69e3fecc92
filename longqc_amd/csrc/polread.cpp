// longqc_amd/csrc/polread.cpp -- host side of the Sequel platform QC (kernels_polread.hpp) behind the C ABI of include/lqcov.h: lqpol_*.
// A handle collects 16-byte items (zmw, start, end, class) on the device -- from inflated BAM bytes (lqpol_add_bytes), from a whole file
// through BGZF pieces (lqpol_add_file) or given directly (lqpol_add_items) -- and lqpol_finish sorts them into the reference's order,
// walks every ZMW and takes N50 / N90.  The per-ZMW arrays stay on the device for lqpol_hist / lqpol_logsum (figdata.cpp's passes).
//
// The records of a piece are found by the device record walk (bamscan.hpp) and read by k_pol_fields.  What the device does not answer for
// goes through pol_twin, this file's own reading of one record, written apart from the kernel's: the records the walk does not vouch for
// (one at a time, from the walk's resume position) and the records k_pol_fields flags.  Where lq_sequel.py itself would raise -- fewer
// than three '/' fields, no '_' piece, text that is no number -- and where a value lies outside what an item holds, pol_twin throws with
// the record's ordinal and name; it never guesses.
#include "lq_cabi.hpp"
#include "bamscan.hpp"
#include "bgzf.hpp"
#include "kernels_crc32.hpp"
#include "kernels_polread.hpp"
#include "figdata_dev.hpp"
#include <cstdlib>
#include <memory>

// reader.cpp: k_bgzf_inflate over a list of BGZF blocks
struct LqDevInflate;
LqDevInflate *lq_dev_inflate_new();
void lq_dev_inflate_free(LqDevInflate *d);
void lq_dev_inflate_run(LqDevInflate *d, hipStream_t stream, const std::vector<BgzfInflater::Block> &blocks, const u8 *win, u8 *d_out, u64 at, std::vector<u32> &status);

namespace {
const char *const KIND[2] = { "scraps", "subreads" };
constexpr u64 POL_PAD = 64;                                   // bytes a device range of BAM bytes extends past its end (the walk's 16-byte loads, the CRC's words)

// blocks of a launch: LQ_POL_MAX_BLOCKS, or fewer with LQPOL_TEST_MAX_BLOCKS (a test hook: the results may not change with it)
u32 max_blocks()
{
	const char *v = getenv("LQPOL_TEST_MAX_BLOCKS");
	const long n = v ? atol(v) : 0;
	return n > 0 && (u64)n < LQ_POL_MAX_BLOCKS ? (u32)n : LQ_POL_MAX_BLOCKS;
}
u32 grid_for(u64 items, u64 per_block = LQ_POL_THREADS)
{
	const u64 g = (items + per_block - 1) / per_block, cap = max_blocks();
	return (u32)(g < 1 ? 1 : g > cap ? cap : g);
}

u32 le32(const u8 *p) { return (u32)p[0] | (u32)p[1] << 8 | (u32)p[2] << 16 | (u32)p[3] << 24; }

std::string where(int kind, u64 rec_no, const std::string &name)
{
	return std::string(KIND[kind]) + " record " + std::to_string(rec_no) + " '" + name + "': ";
}

// ---- the host twin: one whole record rec[0 .. len), len = 4 + block_size, its fixed fields already found consistent ----
struct TwinTag { bool have = false; bool is_char = false; u8 c = 0; };

std::vector<std::string> split(const std::string &s, char sep)
{
	std::vector<std::string> out(1);
	for (char c : s) { if (c == sep) out.emplace_back(); else out.back().push_back(c); }
	return out;
}

u32 twin_int(const std::string &t, const char *what, const std::string &w)
{
	if (t.empty()) throw lq_io_error(w + what + " is empty: not a number");
	size_t k = 0;
	for (char c : t) if (c < '0' || c > '9') throw lq_io_error(w + what + " '" + t + "' is not a plain decimal number");
	while (k + 1 < t.size() && t[k] == '0') ++k;
	if (t.size() - k > LQ_POL_MAX_DIGITS) throw std::domain_error(w + what + " '" + t + "' is above 999999999");
	return (u32)strtoul(t.c_str() + k, nullptr, 10);
}

void twin_aux(const u8 *rec, u64 a, u64 end, TwinTag &sz, TwinTag &sc, const std::string &w)
{
	const auto bad = [&](u64 at, const char *what) { throw lq_io_error(w + "the tag area is malformed at byte " + std::to_string(at) + " of the record: " + what); };
	const auto size_of = [](u8 ty) -> u64 { switch (ty) { case 'A': case 'c': case 'C': return 1; case 's': case 'S': return 2; case 'i': case 'I': case 'f': return 4; case 'd': return 8; default: return 0; } };
	while (a < end) {
		if (a + 3 > end) bad(a, "a tag cut short by the record's end");
		const u8 ty = rec[a + 2];
		const u64 v = a + 3;
		u64 len = size_of(ty);
		if (ty == 'Z' || ty == 'H') {
			const void *nul = memchr(rec + v, 0, (size_t)(end - v));
			if (!nul) bad(a, "a string without its NUL");
			len = (u64)((const u8*)nul - (rec + v)) + 1;
		} else if (ty == 'B') {
			if (v + 5 > end) bad(a, "an array cut short by the record's end");
			const u64 es = rec[v] == 'A' ? 0 : size_of(rec[v]);
			if (!es) bad(a, "an array of an unknown subtype");
			len = 5 + es * (u64)le32(rec + v + 1);
		} else if (!len) bad(a, "an unknown value type");
		if (v + len > end) bad(a, "a value that runs past the record's end");
		TwinTag *t = rec[a] == 's' && rec[a + 1] == 'z' ? &sz : rec[a] == 's' && rec[a + 1] == 'c' ? &sc : nullptr;
		if (t && !t->have) {
			t->have = true;
			// get_tag gives a str for A and for Z alike; a value of any other type equals no letter
			t->is_char = ty == 'A' || (ty == 'Z' && len == 2);
			t->c = rec[v];
		}
		a = v + len;
	}
}

// -> LQ_POL_ITEM (it), LQ_POL_CONTROL (control) or 0
u32 pol_twin(const u8 *rec, u64 len, int kind, u64 rec_no, PolItem &it, i64 &control)
{
	it.zmw = LQ_POL_VOID; it.start = it.end = it.cls = 0; control = 0;
	const u64 l_name = rec[12], n_cigar = (u64)rec[16] | (u64)rec[17] << 8, l_seq = le32(rec + 20);
	const std::string name((const char*)rec + 36, strnlen((const char*)rec + 36, (size_t)l_name));
	const std::string w = where(kind, rec_no, name);
	u32 cls = 'S';
	bool is_control = false;
	if (kind == 0) {
		TwinTag sz, sc;
		twin_aux(rec, 36 + l_name + 4 * n_cigar + (l_seq + 1) / 2 + l_seq, len, sz, sc, w);
		if (!sz.have || !sc.have) return 0;
		if (!sz.is_char) return 0;
		if (sz.c == 'C') is_control = true;
		else if (sz.c != 'N') return 0;
		cls = sc.is_char ? sc.c : LQ_POL_CLASS_OTHER;
	}
	const std::vector<std::string> f = split(name, '/');
	if (f.size() < 3) throw lq_io_error(w + "the name has fewer than three '/' fields");
	if (is_control && cls != 'F') return 0;
	const std::vector<std::string> pos = split(f[2], '_');
	if (pos.size() < 2) throw lq_io_error(w + "the name's third field has no '_'");
	const u32 start = twin_int(pos[0], "start", w), end = twin_int(pos[1], "end", w);
	if (is_control) { control = (i64)end - (i64)start + 1; return LQ_POL_CONTROL; }
	const std::string &z = f[1];
	bool plain = !z.empty() && z.size() <= LQ_POL_MAX_DIGITS && !(z[0] == '0' && z.size() > 1);
	for (char c : z) plain = plain && c >= '0' && c <= '9';
	if (!plain) throw std::domain_error(w + "the ZMW '" + z + "' is not a number of 1 to 9 digits without leading zeros (ZMWs are told apart by their text)");
	it.zmw = (u32)strtoul(z.c_str(), nullptr, 10); it.start = start; it.end = end; it.cls = cls;
	return LQ_POL_ITEM;
}

// the fixed fields of a record that the device walk does not vouch for, as reader.cpp's parse_bam_one checks them: h[0 .. have), have >= 36
// -> 4 + block_size
u64 host_record_len(const u8 *h, int kind, u64 rec_no)
{
	const std::string w = std::string(KIND[kind]) + " record " + std::to_string(rec_no) + ": ";
	const u64 block_size = le32(h), l_name = h[12], n_cigar = (u64)h[16] | (u64)h[17] << 8, l_seq = le32(h + 20);
	if (l_seq > 0x7fffffffULL) throw std::domain_error(w + "read longer than 2^31-1 bases");
	const u64 fields = 32 + l_name + 4 * n_cigar + (l_seq + 1) / 2 + l_seq;
	if (block_size > 0x7fffffffULL || block_size < fields) throw lq_io_error(w + "block_size " + std::to_string((i32)block_size) + " is too small for its fields (" + std::to_string(fields) + " bytes)");
	if (l_name == 0) throw lq_io_error(w + "l_read_name is 0");
	return 4 + block_size;
}
} // namespace

struct lqpol {
	int device = 0;
	hipStream_t stream = nullptr;
	std::string err;
	int state = 0;                                            // 0: scraps may come, 1: subreads have come, 2: finished
	Prim prim;
	DBuf items; u64 n_items = 0, n_void = 0;
	i64 control = 0;
	u64 rec_no[2] = {0, 0};
	std::string header[2];
	u64 st_device = 0, st_twin = 0, st_hostwalk = 0, st_inflated = 0, st_to_host = 0, st_pieces = 0;
	BamScan scan;
	DBuf d_bytes, tmp, flags, cols, ctl;
	std::vector<u32> h_flags; std::vector<FxRow> h_rows; std::vector<u8> h_rec;
	bool timing = false; double t_scan = 0, t_fields = 0;     // LQCOV_TIMING: the record stage's two parts, each closed by a wait
	// the result
	DBuf z, hq, tot, ad, pol, hq32, tot32, ad32;
	u64 n_zmw = 0, n_pol = 0, n_long = 0;
	PolSums sums;

	~lqpol() { if (stream) (void)hipStreamDestroy(stream); }

	void items_room(u64 more)
	{
		if (n_items + more >= (1ULL << 32) - 1) throw std::domain_error("2^32 items or more");
		const size_t need = (size_t)(n_items + more) * sizeof(PolItem), kept = (size_t)n_items * sizeof(PolItem);
		items.grow(need, std::max(need, 2 * kept), kept, stream);
	}

	void put_item(u64 at, const PolItem &it)
	{
		LQ_HIP_CHECK(hipMemcpyAsync(items.as<PolItem>() + at, &it, sizeof(PolItem), hipMemcpyHostToDevice, stream));
		LQ_HIP_CHECK(hipStreamSynchronize(stream));
	}

	// len bytes at position `at` of the range: the host's own (h) or fetched from the device's (d)
	const u8 *host_view(const u8 *d, const u8 *h, u64 at, u64 len)
	{
		if (h) return h + at;
		h_rec.resize((size_t)len);
		LQ_HIP_CHECK(hipMemcpyAsync(h_rec.data(), d + at, (size_t)len, hipMemcpyDeviceToHost, stream));
		LQ_HIP_CHECK(hipStreamSynchronize(stream));
		st_to_host += len;
		return h_rec.data();
	}

	void add_kind(int kind)
	{
		if (kind != 0 && kind != 1) throw std::invalid_argument("kind is neither 0 (scraps) nor 1 (subreads)");
		if (state == 2) throw std::logic_error("the handle is finished");
		if (kind == 0 && state == 1) throw std::logic_error("scraps after subreads: the scraps file comes first (its items arrive first)");
		if (kind == 1) state = 1;
	}

	// k_pol_fields over the rows of the last scan of d[0 .. n)
	void fields(const u8 *d, const u8 *h, int kind)
	{
		const u64 n = scan.n_rows, n_tiles = (n + LQ_FXSCAN_LINE_TILE - 1) / LQ_FXSCAN_LINE_TILE;
		tmp.ensure((size_t)n * sizeof(PolItem)); flags.ensure((size_t)n * 4); cols.ensure((size_t)n_tiles * 8); ctl.ensure(32);
		LQ_HIP_CHECK(hipMemsetAsync(ctl.p, 0, 32, stream));
		LQ_LAUNCH(k_pol_fields, grid_for(n_tiles, 1), LQ_POL_THREADS, stream, d, 0u, (const FxRow*)scan.rows.as<FxRow>(), n, kind, tmp.as<PolItem>(), flags.as<u32>(), cols.as<u64>(),
		          ctl.as<unsigned long long>());
		LQ_LAUNCH(k_fx_tilescan, 1, LQ_FXSCAN_THREADS, stream, cols.as<u64>(), n_tiles, 1u, ctl.as<u64>() + 2);
		LQ_HIP_CHECK(hipGetLastError());
		u64 c[3];
		LQ_HIP_CHECK(hipMemcpyAsync(c, ctl.p, 24, hipMemcpyDeviceToHost, stream));
		LQ_HIP_CHECK(hipStreamSynchronize(stream));
		const u64 slots = c[2], flagged = c[1];
		control += (i64)c[0];
		items_room(slots);
		if (slots) LQ_LAUNCH(k_pol_compact, grid_for(n_tiles, 1), LQ_POL_THREADS, stream, (const PolItem*)tmp.as<PolItem>(), (const u32*)flags.as<u32>(), n, (const u64*)cols.as<u64>(), items.as<PolItem>() + n_items);
		LQ_HIP_CHECK(hipGetLastError());
		if (flagged) {                                            // the twin fills the flagged records' slots in
			h_flags.resize((size_t)n); h_rows.resize((size_t)n);       // (the scan leaves its rows on the device: they come with the flags, here alone)
			LQ_HIP_CHECK(hipMemcpyAsync(h_flags.data(), flags.p, (size_t)n * 4, hipMemcpyDeviceToHost, stream));
			LQ_HIP_CHECK(hipMemcpyAsync(h_rows.data(), scan.rows.p, (size_t)n * sizeof(FxRow), hipMemcpyDeviceToHost, stream));
			LQ_HIP_CHECK(hipStreamSynchronize(stream));
			st_to_host += n * (4 + sizeof(FxRow));
			u64 slot = n_items;
			for (u64 r = 0; r < n; ++r) {
				const u32 f = h_flags[r];
				if (f & LQ_POL_FLAGGED) {
					const u64 at = h_rows[r].name_at - 36;
					const u64 len = 4 + (u64)le32(host_view(d, h, at, 4));
					PolItem it; i64 c1;
					const u32 got = pol_twin(host_view(d, h, at, len), len, kind, rec_no[kind] + r + 1, it, c1);
					control += c1;
					if (got & LQ_POL_ITEM) put_item(slot, it); else ++n_void;
					++st_twin;
				}
				if (f & (LQ_POL_ITEM | LQ_POL_FLAGGED)) ++slot;
			}
		}
		n_items += slots;
		rec_no[kind] += n; st_device += n - flagged;
		if (timing) LQ_HIP_CHECK(hipStreamSynchronize(stream));
	}

	// the records of d[start .. n) (h: the same bytes on the host, or null) -> the position of the first record that is not whole
	u64 range(const u8 *d, const u8 *h, u64 n, u64 start, int kind)
	{
		u64 pos = start, host_run = 1;
		while (pos < n) {
			if (timing) LQ_HIP_CHECK(hipStreamSynchronize(stream));   // (the upload or the inflate before is not the scan's)
			const double t0 = lq_now_s();
			scan.run_bam(stream, d, n, pos, false);
			const double t1 = lq_now_s();
			if (scan.n_rows) { fields(d, h, kind); host_run = 1; }
			t_scan += t1 - t0; t_fields += lq_now_s() - t1;
			pos = scan.resume_pos;
			// what the walk does not vouch for: 1, 2, 4 .. records by the host between two scans
			u64 done = 0;
			for (; done < host_run && pos < n; ++done) {
				if (n - pos < 36) return pos;
				const u64 len = host_record_len(host_view(d, h, pos, 36), kind, rec_no[kind] + 1);
				if (n - pos < len) return pos;
				const u8 *rec = host_view(d, h, pos, len);
				if (rec[36 + rec[12] - 1] != 0) throw lq_io_error(std::string(KIND[kind]) + " record " + std::to_string(rec_no[kind] + 1) + ": the read name has no NUL at its end");
				PolItem it; i64 c1;
				const u32 got = pol_twin(rec, len, kind, rec_no[kind] + 1, it, c1);
				control += c1;
				if (got & LQ_POL_ITEM) { items_room(1); put_item(n_items, it); ++n_items; }
				++rec_no[kind]; ++st_hostwalk;
				pos += len;
			}
			if (done == host_run && scan.n_rows == 0) host_run = std::min<u64>(host_run * 2, 1u << 16);
		}
		return pos;
	}

	void add_bytes(int kind, const u8 *bytes, u64 n, u64 start_pos, u64 *resume)
	{
		add_kind(kind);
		if (start_pos > n) throw std::invalid_argument("no parser state");
		if (n >= LQ_FXSCAN_MAX_BYTES - POL_PAD) throw std::domain_error("a range of 2^32 bytes or more");
		*resume = start_pos;
		if (start_pos >= n) return;
		d_bytes.ensure((size_t)(n + POL_PAD));
		LQ_HIP_CHECK(hipMemcpyAsync(d_bytes.p, bytes, (size_t)n, hipMemcpyHostToDevice, stream));
		LQ_HIP_CHECK(hipMemsetAsync(d_bytes.as<u8>() + n, 0, POL_PAD, stream));
		*resume = range(d_bytes.as<u8>(), bytes, n, start_pos, kind);
	}

	void add_items(const u32 *zmw, const u32 *start, const u32 *end, const u8 *cls, u64 n)
	{
		if (state == 2) throw std::logic_error("the handle is finished");
		if (!n) return;
		if (!zmw || !start || !end || !cls) throw std::invalid_argument("null buffers");
		std::vector<PolItem> h((size_t)n);
		for (u64 i = 0; i < n; ++i) {
			if (zmw[i] > 999999999u || start[i] > 999999999u || end[i] > 999999999u) throw std::domain_error("item " + std::to_string(i) + ": a value above 999999999");
			h[i] = { zmw[i], start[i], end[i], cls[i] };
		}
		items_room(n);
		LQ_HIP_CHECK(hipMemcpyAsync(items.as<PolItem>() + n_items, h.data(), (size_t)n * sizeof(PolItem), hipMemcpyHostToDevice, stream));
		LQ_HIP_CHECK(hipStreamSynchronize(stream));
		n_items += n;
	}

	// LQPOL_PIECE_BYTES: the size of a piece (tests: pieces shorter than a ZMW's records)
	static u64 piece_bytes()
	{
		const char *e = getenv("LQPOL_PIECE_BYTES");
		const u64 v = e ? strtoull(e, nullptr, 10) : 0;
		return v ? std::max<u64>(v, 64) : (u64)32 << 20;
	}

	// the whole file, piece by piece: h[0 .. fill) / d[0 .. fill) hold the inflated bytes from the first one not consumed yet
	void add_file(int kind, const std::string &path, int inflate_mode, int host_copy)
	{
		add_kind(kind);
		if (inflate_mode != LQREADER_INFLATE_HOST && inflate_mode != LQREADER_INFLATE_DEVICE) throw std::invalid_argument("inflate mode");
		if (host_copy != LQREADER_HOSTCOPY_ALL && host_copy != LQREADER_HOSTCOPY_NEEDED) throw std::invalid_argument("host copy mode");
		const bool dev = inflate_mode == LQREADER_INFLATE_DEVICE, keep = dev && host_copy == LQREADER_HOSTCOPY_NEEDED;
		struct Fd { int fd = -1; ~Fd() { if (fd >= 0) ::close(fd); } } f;
		f.fd = ::open(path.c_str(), O_RDONLY);
		if (f.fd < 0) throw lq_open_error(path);
		BgzfInflater z; z.fd = f.fd; z.n_threads = 8;
		u64 cap = piece_bytes(), fill = 0, pos = 0;
		std::unique_ptr<u8[]> h(new u8[cap]);                     // not filled: with `keep` only its addresses are used, no page of it is touched
		DBuf d_cur, d_next;
		d_cur.ensure((size_t)(cap + POL_PAD));
		std::unique_ptr<LqDevInflate, void (*)(LqDevInflate*)> inf(dev ? lq_dev_inflate_new() : nullptr, lq_dev_inflate_free);
		CrcDev crc;
		if (dev) z.device = [&](const std::vector<BgzfInflater::Block> &blocks, const u8 *win, u8 *dst, u64 out_bytes, std::vector<u32> &status) {
			const u64 at = (u64)(dst - h.get());
			lq_dev_inflate_run(inf.get(), stream, blocks, win, d_cur.as<u8>(), at, status);
			if (keep) {
				std::vector<u64> off(blocks.size()), len(blocks.size());
				for (size_t i = 0; i < blocks.size(); ++i) { off[i] = at + blocks[i].out; len[i] = blocks[i].isize; }
				z.dev_crc.assign(blocks.size(), 0);
				crc.run(stream, d_cur.as<u8>(), (u32)blocks.size(), off.data(), len.data(), z.dev_crc.data());
				return;
			}
			if (out_bytes) LQ_HIP_CHECK(hipMemcpyAsync(dst, d_cur.as<u8>() + at, (size_t)out_bytes, hipMemcpyDeviceToHost, stream));
			LQ_HIP_CHECK(hipStreamSynchronize(stream));
			st_to_host += out_bytes;
		};
		const auto grow = [&](u64 want) {                         // a header or a record longer than the piece
			d_next.ensure((size_t)(want + POL_PAD));
			if (fill) LQ_HIP_CHECK(hipMemcpyAsync(d_next.p, d_cur.p, (size_t)fill, hipMemcpyDeviceToDevice, stream));
			LQ_HIP_CHECK(hipStreamSynchronize(stream));
			d_cur.swap(d_next);
			std::unique_ptr<u8[]> nh(new u8[want]);
			if (!keep && fill) memcpy(nh.get(), h.get(), (size_t)fill);
			h.swap(nh); cap = want;
		};
		bool in_header = true;
		const auto fail = [&](const std::string &what) { throw lq_open_error(path, what); };
		for (;;) {
			u64 need = 0;
			try {
				while (!z.ended) {
					const u64 got = z.fill(h.get() + fill, cap - fill, &need);
					if (!got) break;
					if (!dev) LQ_HIP_CHECK(hipMemcpyAsync(d_cur.as<u8>() + fill, h.get() + fill, (size_t)got, hipMemcpyHostToDevice, stream));
					fill += got; st_inflated += got;
				}
			} catch (const lq_file_error &e) { fail(e.what()); }
			LQ_HIP_CHECK(hipMemsetAsync(d_cur.as<u8>() + fill, 0, POL_PAD, stream));
			LQ_HIP_CHECK(hipStreamSynchronize(stream));
			++st_pieces;
			const u8 *hv = keep ? nullptr : h.get();
			if (in_header) {                                       // magic, l_text, text, n_ref, per reference l_name, name, l_ref
				u64 q = 0; bool whole = false;
				do {
					if (fill < 12) break;
					const u8 *p8 = host_view(d_cur.as<u8>(), hv, 0, 8);
					if (memcmp(p8, "BAM\1", 4) != 0) fail("not a BAM file");
					const u64 l_text = le32(p8 + 4);
					if (fill < 12 + l_text) break;
					const u8 *t = host_view(d_cur.as<u8>(), hv, 8, l_text + 4);
					header[kind].assign((const char*)t, (size_t)l_text);
					u64 refs = le32(t + l_text);
					q = 12 + l_text;
					while (refs && fill >= q + 4) {
						const u64 l_name = le32(host_view(d_cur.as<u8>(), hv, q, 4));
						if (fill < q + 8 + l_name) break;
						q += 8 + l_name; --refs;
					}
					whole = refs == 0;
				} while (false);
				if (whole) { pos = q; in_header = false; }
				else if (z.ended) fail("the file ends inside the BAM header");
			}
			if (!in_header) {
				try { pos = range(d_cur.as<u8>(), hv, fill, pos, kind); }
				catch (const lq_io_error &e) { fail(e.what()); }
			}
			if (z.ended) {
				if (pos < fill) fail(std::string(KIND[kind]) + " record " + std::to_string(rec_no[kind] + 1) + ": the file ends inside a record");
				break;
			}
			if (pos) {                                             // what is left moves to the front of the other block
				const u64 rem = fill - pos;
				d_next.ensure((size_t)(cap + POL_PAD));
				if (rem) LQ_HIP_CHECK(hipMemcpyAsync(d_next.p, d_cur.as<u8>() + pos, (size_t)rem, hipMemcpyDeviceToDevice, stream));
				LQ_HIP_CHECK(hipStreamSynchronize(stream));
				d_cur.swap(d_next);
				if (!keep && rem) memmove(h.get(), h.get() + pos, (size_t)rem);
				fill = rem; pos = 0;
			}
			if (cap - fill < need) grow(std::max(cap * 2, fill + need));      // a header or a record longer than the piece
		}
	}

	void finish()
	{
		if (state == 2) throw std::logic_error("the handle is finished");
		state = 2;
		n_zmw = n_pol = n_long = 0;
		PolSums init = {0, 0, ~0ULL, 0, 0, 0, 0xffffffffu, 0, 0, 0};
		sums = init;
		const u64 n = n_items, nv = n_items - n_void;
		if (!nv) return;
		// LQCOV_TIMING: the call's stages on stderr, each closed by a wait for the stream (the waits are the timing's, not the call's)
		if (timing) fprintf(stderr, "lqpol records: %llu by the device: record walk %.3f k_pol_fields+compact %.3f ms\n", (unsigned long long)st_device, t_scan * 1e3, t_fields * 1e3);
		double t_last = lq_now_s(), t_stage[3] = {0, 0, 0};
		const auto stage = [&](int k) {
			if (!timing) return;
			LQ_HIP_CHECK(hipStreamSynchronize(stream));
			const double now = lq_now_s(); t_stage[k] += now - t_last; t_last = now;
		};
		struct Report { const bool on; const u64 n; const u64 &zmw; const double *t; ~Report() { if (on) fprintf(stderr, "lqpol_finish: %llu items %llu ZMWs: keys+sort %.3f order+heads+walk %.3f pack+N50/N90 %.3f ms\n",
			(unsigned long long)n, (unsigned long long)zmw, t[0] * 1e3, t[1] * 1e3, t[2] * 1e3); } } report{timing, n, n_zmw, t_stage};
		const PolItem *it = items.as<PolItem>();
		DBuf k_end, k_end_s, idx0, idx1, idx2, k_zs, k2, k2s, sorted, flag, pos, head, long_list, ctl2, isp, ppos, key, key_s, v, ex, d_sums;
		k_end.ensure((size_t)n * 4); k_end_s.ensure((size_t)n * 4); idx0.ensure((size_t)n * 8); idx1.ensure((size_t)n * 8); idx2.ensure((size_t)n * 8);
		k_zs.ensure((size_t)n * 8); k2.ensure((size_t)n * 8); k2s.ensure((size_t)n * 8);
		LQ_LAUNCH(k_pol_keys, grid_for(n), LQ_POL_THREADS, stream, it, n, k_end.as<u32>(), idx0.as<u64>(), k_zs.as<u64>());
		prim.radix<u32, u64, true>(k_end.as<u32>(), k_end_s.as<u32>(), idx0.as<u64>(), idx1.as<u64>(), (size_t)n, 30);
		LQ_LAUNCH(k_pol_rekey, grid_for(n), LQ_POL_THREADS, stream, (const u64*)k_zs.as<u64>(), (const u64*)idx1.as<u64>(), n, k2.as<u64>());
		prim.radix<u64, u64, true>(k2.as<u64>(), k2s.as<u64>(), idx1.as<u64>(), idx2.as<u64>(), (size_t)n, 63);
		stage(0);
		sorted.ensure((size_t)nv * sizeof(PolItem)); flag.ensure((size_t)(nv + 1) * 4); pos.ensure((size_t)(nv + 1) * 4);
		LQ_LAUNCH(k_pol_order, grid_for(nv + 1), LQ_POL_THREADS, stream, it, (const u64*)k2s.as<u64>(), (const u64*)idx2.as<u64>(), nv, sorted.as<PolItem>(), flag.as<u32>());
		LQ_HIP_CHECK(hipGetLastError());
		prim.exclusive_scan_u32_u32(flag.as<u32>(), pos.as<u32>(), (size_t)nv + 1);
		u32 groups = 0;
		LQ_HIP_CHECK(hipMemcpyAsync(&groups, pos.as<u32>() + nv, 4, hipMemcpyDeviceToHost, stream));
		LQ_HIP_CHECK(hipStreamSynchronize(stream));
		if (groups < 1 || groups > nv) throw std::logic_error("the ZMWs' heads do not fit the items");
		head.ensure((size_t)(groups + 1) * 4); long_list.ensure((size_t)groups * 4); ctl2.ensure(8);
		z.ensure((size_t)groups * 4); hq.ensure((size_t)groups * 8); tot.ensure((size_t)groups * 8); ad.ensure((size_t)groups * 4); pol.ensure((size_t)groups * 4);
		LQ_HIP_CHECK(hipMemsetAsync(ctl2.p, 0, 8, stream));
		LQ_LAUNCH(k_pol_heads, grid_for(nv), LQ_POL_THREADS, stream, (const u32*)flag.as<u32>(), (const u32*)pos.as<u32>(), nv, head.as<u32>());
		LQ_LAUNCH(k_pol_walk, grid_for(groups), LQ_POL_THREADS, stream, (const PolItem*)sorted.as<PolItem>(), (const u32*)head.as<u32>(), (u64)groups, (const u32*)nullptr, long_list.as<u32>(),
		          ctl2.as<u32>(), z.as<u32>(), hq.as<i64>(), tot.as<i64>(), ad.as<u32>(), pol.as<u32>());
		LQ_HIP_CHECK(hipGetLastError());
		u32 n_lng = 0;
		LQ_HIP_CHECK(hipMemcpyAsync(&n_lng, ctl2.p, 4, hipMemcpyDeviceToHost, stream));
		LQ_HIP_CHECK(hipStreamSynchronize(stream));
		if (n_lng) LQ_LAUNCH(k_pol_walk, grid_for(n_lng), LQ_POL_THREADS, stream, (const PolItem*)sorted.as<PolItem>(), (const u32*)head.as<u32>(), (u64)n_lng, (const u32*)long_list.as<u32>(), (u32*)nullptr,
		                     (u32*)nullptr, z.as<u32>(), hq.as<i64>(), tot.as<i64>(), ad.as<u32>(), pol.as<u32>());
		isp.ensure((size_t)(groups + 1) * 4); ppos.ensure((size_t)(groups + 1) * 4);
		LQ_LAUNCH(k_pol_ispol, grid_for((u64)groups + 1), LQ_POL_THREADS, stream, (const u32*)pol.as<u32>(), (u64)groups, isp.as<u32>());
		LQ_HIP_CHECK(hipGetLastError());
		prim.exclusive_scan_u32_u32(isp.as<u32>(), ppos.as<u32>(), (size_t)groups + 1);
		u32 np = 0;
		LQ_HIP_CHECK(hipMemcpyAsync(&np, ppos.as<u32>() + groups, 4, hipMemcpyDeviceToHost, stream));
		LQ_HIP_CHECK(hipStreamSynchronize(stream));
		n_zmw = groups; n_long = n_lng; n_pol = np;
		stage(1);
		if (!np) return;
		hq32.ensure((size_t)np * 4); tot32.ensure((size_t)np * 4); ad32.ensure((size_t)np * 4);
		key.ensure((size_t)np * 4); key_s.ensure((size_t)np * 4); v.ensure((size_t)np * 4); ex.ensure((size_t)np * 8); d_sums.ensure(sizeof(PolSums));
		LQ_HIP_CHECK(hipMemcpyAsync(d_sums.p, &init, sizeof(PolSums), hipMemcpyHostToDevice, stream));
		LQ_LAUNCH(k_pol_pack, grid_for(groups), LQ_POL_THREADS, stream, (const i64*)hq.as<i64>(), (const i64*)tot.as<i64>(), (const u32*)ad.as<u32>(), (const u32*)pol.as<u32>(), (const u32*)ppos.as<u32>(),
		          (u64)groups, hq32.as<u32>(), tot32.as<u32>(), ad32.as<u32>(), key.as<u32>(), d_sums.as<PolSums>());
		LQ_HIP_CHECK(hipGetLastError());
		prim.sort_keys_u32(key.as<u32>(), key_s.as<u32>(), (size_t)np);
		LQ_LAUNCH(k_pol_unkey, grid_for(np), LQ_POL_THREADS, stream, (const u32*)key_s.as<u32>(), (u64)np, v.as<u32>());
		LQ_HIP_CHECK(hipGetLastError());
		prim.exclusive_scan_u32_u64(v.as<u32>(), ex.as<u64>(), (size_t)np);
		LQ_LAUNCH(k_pol_nxx, grid_for(np), LQ_POL_THREADS, stream, (const u32*)v.as<u32>(), (const u64*)ex.as<u64>(), (u64)np, d_sums.as<PolSums>());
		LQ_HIP_CHECK(hipGetLastError());
		LQ_HIP_CHECK(hipMemcpyAsync(&sums, d_sums.p, sizeof(PolSums), hipMemcpyDeviceToHost, stream));
		LQ_HIP_CHECK(hipStreamSynchronize(stream));
		stage(2);
		if (sums.n_range) return;                                 // (need_lengths refuses the sums and the resident arrays; the per-ZMW integers stand)
		if (sums.sum_hq >= (1ULL << 53) / 100) throw std::domain_error("100 times the throughput reaches 2^53: N50 and N90 by integers would no longer be the reference's");
	}

	void need_finished() const { if (state != 2) throw std::logic_error("lqpol_finish has not been called"); }
	// the uint32 arrays of the is_pol ZMWs hold every length
	void need_lengths() const
	{
		need_finished();
		if (sums.n_range) throw std::domain_error(std::to_string(sums.n_range) + " polymerase reads with a length below 0 or above 2^32-1");
	}
};

namespace {
template <class F> int pol_call(lqpol *p, F &&f)
{
	if (!p) return LQCOV_E_ARG;
	char msg[768] = {0};
	const int rc = lq_cabi::guarded(msg, sizeof(msg), [&] {
		lq_cabi::select_device(p->device);
		try { f(); }
		catch (...) { (void)hipStreamSynchronize(p->stream); throw; }
	});
	if (rc) p->err = msg;
	return rc;
}
thread_local std::string g_pol_error;
} // namespace

extern "C" {

lqpol *lqpol_create(int device)
{
	try {
		lq_cabi::select_device(device);
		std::unique_ptr<lqpol> p(new lqpol());
		p->device = device;
		LQ_HIP_CHECK(hipStreamCreate(&p->stream));
		p->prim.stream = p->stream;
		p->scan.fetch_rows = false;
		p->timing = getenv("LQCOV_TIMING") != nullptr;
		return p.release();
	} catch (const std::exception &e) { g_pol_error = e.what(); return nullptr; }
}

void lqpol_destroy(lqpol *p) { delete p; }

const char *lqpol_last_error(const lqpol *p) { return p ? p->err.c_str() : g_pol_error.c_str(); }

int lqpol_add_bytes(lqpol *p, int kind, const uint8_t *bytes, uint64_t n, uint64_t start_pos, uint64_t *resume_pos)
{
	return pol_call(p, [&] {
		if (!resume_pos || (n && !bytes)) throw std::invalid_argument("null buffers");
		p->add_bytes(kind, bytes, n, start_pos, resume_pos);
	});
}

int lqpol_add_file(lqpol *p, int kind, const char *path, int inflate_mode, int host_copy_mode)
{
	return pol_call(p, [&] {
		if (!path) throw std::invalid_argument("null path");
		p->add_file(kind, path, inflate_mode, host_copy_mode);
	});
}

int lqpol_file_header(const char *path, char *buf, uint64_t cap, uint64_t *len, char *errbuf, size_t errbuf_len)
{
	return lq_cabi::guarded(errbuf, errbuf_len, [&] {
		if (!path || !len) throw std::invalid_argument("null buffers");
		struct Fd { int fd = -1; ~Fd() { if (fd >= 0) ::close(fd); } } f;
		f.fd = ::open(path, O_RDONLY);
		if (f.fd < 0) throw lq_open_error(path);
		BgzfInflater z; z.fd = f.fd;
		std::vector<u8> h;
		u64 fill = 0, want = 8;                                   // magic and l_text, then the text
		try {
			while (fill < want) {
				h.resize((size_t)(fill + BgzfInflater::MAX_BLOCK));
				u64 need = 0;
				const u64 got = z.fill(h.data() + fill, BgzfInflater::MAX_BLOCK, &need, 1);
				if (!got && z.ended) throw lq_file_error("the file ends inside the BAM header");
				fill += got;
				if (fill >= 8) {
					if (memcmp(h.data(), "BAM\1", 4) != 0) throw lq_file_error("not a BAM file");
					want = 8 + (u64)le32(h.data() + 4);
				}
			}
		} catch (const lq_file_error &e) { throw lq_open_error(path, e.what()); }
		*len = want - 8;
		if (buf && cap) memcpy(buf, h.data() + 8, (size_t)std::min<u64>(cap, want - 8));
	});
}

int lqpol_header_text(const lqpol *p, int kind, char *buf, uint64_t cap, uint64_t *len)
{
	if (!p || !len || (kind != 0 && kind != 1)) return LQCOV_E_ARG;
	const std::string &t = p->header[kind];
	*len = t.size();
	if (buf && cap) memcpy(buf, t.data(), (size_t)std::min<u64>(cap, t.size()));
	return 0;
}

int lqpol_add_items(lqpol *p, const uint32_t *zmw, const uint32_t *start, const uint32_t *end, const uint8_t *cls, uint64_t n)
{
	return pol_call(p, [&] { p->add_items(zmw, start, end, cls, n); });
}

int lqpol_finish(lqpol *p, uint64_t *n_zmw, uint64_t *n_pol, int64_t *control)
{
	return pol_call(p, [&] {
		if (!n_zmw || !n_pol || !control) throw std::invalid_argument("null buffers");
		p->finish();
		*n_zmw = p->n_zmw; *n_pol = p->n_pol; *control = p->control;
	});
}

int lqpol_get(lqpol *p, uint32_t *zmw, int64_t *hq, int64_t *tot, uint32_t *ad, uint8_t *is_pol)
{
	return pol_call(p, [&] {
		p->need_finished();
		const u64 n = p->n_zmw;
		if (!n) return;
		if (zmw) LQ_HIP_CHECK(hipMemcpyAsync(zmw, p->z.p, (size_t)n * 4, hipMemcpyDeviceToHost, p->stream));
		if (hq) LQ_HIP_CHECK(hipMemcpyAsync(hq, p->hq.p, (size_t)n * 8, hipMemcpyDeviceToHost, p->stream));
		if (tot) LQ_HIP_CHECK(hipMemcpyAsync(tot, p->tot.p, (size_t)n * 8, hipMemcpyDeviceToHost, p->stream));
		if (ad) LQ_HIP_CHECK(hipMemcpyAsync(ad, p->ad.p, (size_t)n * 4, hipMemcpyDeviceToHost, p->stream));
		std::vector<u32> pol;
		if (is_pol) { pol.resize((size_t)n); LQ_HIP_CHECK(hipMemcpyAsync(pol.data(), p->pol.p, (size_t)n * 4, hipMemcpyDeviceToHost, p->stream)); }
		LQ_HIP_CHECK(hipStreamSynchronize(p->stream));
		if (is_pol) for (u64 g = 0; g < n; ++g) is_pol[g] = (u8)(pol[g] & 1u);
	});
}

int lqpol_stats(const lqpol *p, uint64_t out[LQPOL_STATS_WORDS])
{
	if (!p || !out || p->state != 2) return p && out ? LQCOV_E_STATE : LQCOV_E_ARG;
	const PolSums &s = p->sums;
	const bool some = p->n_pol != 0;
	const uint64_t v[LQPOL_STATS_WORDS] = { s.sum_hq, s.max_hq, some ? s.min_tot : 0, s.max_tot, s.n50, s.n90, s.n_flagged, some ? s.min_ad : 0, s.max_ad, p->n_long,
	                                        p->st_device, p->st_twin, p->st_hostwalk, p->st_inflated, p->st_to_host, p->st_pieces, s.n_range };
	memcpy(out, v, sizeof(v));
	return 0;
}

int lqpol_hist(lqpol *p, int which, const double *edges, uint32_t n_edges, uint64_t *counts)
{
	return pol_call(p, [&] {
		p->need_lengths();
		if (which < LQPOL_HQ || which > LQPOL_AD) throw std::invalid_argument("which is none of LQPOL_HQ, LQPOL_TOT, LQPOL_AD");
		if (n_edges && !edges) throw std::invalid_argument("null buffers");
		for (u32 k = 0; k < n_edges; ++k)
			if (edges[k] != edges[k] || (k && edges[k] < edges[k - 1])) throw std::invalid_argument("edges are not ascending");
		if (n_edges < 2) return;
		if (!counts) throw std::invalid_argument("null buffers");
		for (u32 k = 0; k + 1 < n_edges; ++k) counts[k] = 0;
		if (!p->n_pol) return;
		const DBuf &x = which == LQPOL_HQ ? p->hq32 : which == LQPOL_TOT ? p->tot32 : p->ad32;
		lq_fig_hist_dev(p->stream, LQFIG_U32, x.p, p->n_pol, edges, n_edges, counts);
	});
}

int lqpol_logsum(lqpol *p, uint64_t *sum, double *sum_log, uint64_t *n_zero)
{
	return pol_call(p, [&] {
		p->need_lengths();
		if (!sum || !sum_log || !n_zero) throw std::invalid_argument("null buffers");
		*sum = 0; *sum_log = 0.0; *n_zero = 0;
		if (!p->n_pol) return;
		lq_fig_logsum_dev(p->stream, p->hq32.as<u32>(), p->n_pol, sum, sum_log, n_zero);
	});
}

int lqpol_fields(int device, int kind, const uint8_t *bytes, uint64_t n, uint64_t start_pos, uint32_t *flags, uint32_t *items, uint64_t cap,
                 uint64_t *n_rows, uint64_t *n_slots, int64_t *control, uint64_t *resume_pos, char *errbuf, size_t errbuf_len)
{
	return lq_cabi::guarded(errbuf, errbuf_len, [&] {
		if (!n_rows || !n_slots || !control || !resume_pos || (n && !bytes)) throw std::invalid_argument("null buffers");
		if (kind != 0 && kind != 1) throw std::invalid_argument("kind is neither 0 (scraps) nor 1 (subreads)");
		if (start_pos > n) throw std::invalid_argument("no parser state");
		if (n >= LQ_FXSCAN_MAX_BYTES - POL_PAD) throw std::domain_error("a range of 2^32 bytes or more");
		*n_rows = *n_slots = 0; *control = 0; *resume_pos = start_pos;
		if (start_pos >= n) return;
		lq_cabi::ScopedStream s(device);
		DBuf d, tmp, fl, cols, ctl, out;
		d.ensure((size_t)(n + POL_PAD));
		LQ_HIP_CHECK(hipMemcpyAsync(d.p, bytes, (size_t)n, hipMemcpyHostToDevice, s));
		LQ_HIP_CHECK(hipMemsetAsync(d.as<u8>() + n, 0, POL_PAD, s));
		BamScan bs;
		bs.fetch_rows = false;
		bs.run_bam(s, d.as<u8>(), n, start_pos, false);
		*resume_pos = bs.resume_pos; *n_rows = bs.n_rows;
		const u64 nr = bs.n_rows, n_tiles = (nr + LQ_FXSCAN_LINE_TILE - 1) / LQ_FXSCAN_LINE_TILE;
		if (!nr) return;
		if (nr > cap || !flags || !items) throw std::invalid_argument("the tables are smaller than the scan's result");
		tmp.ensure((size_t)nr * sizeof(PolItem)); fl.ensure((size_t)nr * 4); cols.ensure((size_t)n_tiles * 8); ctl.ensure(32); out.ensure((size_t)nr * sizeof(PolItem));
		LQ_HIP_CHECK(hipMemsetAsync(ctl.p, 0, 32, s));
		LQ_LAUNCH(k_pol_fields, grid_for(n_tiles, 1), LQ_POL_THREADS, s, (const u8*)d.as<u8>(), 0u, (const FxRow*)bs.rows.as<FxRow>(), nr, kind, tmp.as<PolItem>(), fl.as<u32>(), cols.as<u64>(),
		          ctl.as<unsigned long long>());
		LQ_LAUNCH(k_fx_tilescan, 1, LQ_FXSCAN_THREADS, s, cols.as<u64>(), n_tiles, 1u, ctl.as<u64>() + 2);
		LQ_LAUNCH(k_pol_compact, grid_for(n_tiles, 1), LQ_POL_THREADS, s, (const PolItem*)tmp.as<PolItem>(), (const u32*)fl.as<u32>(), nr, (const u64*)cols.as<u64>(), out.as<PolItem>());
		LQ_HIP_CHECK(hipGetLastError());
		u64 c[3];
		LQ_HIP_CHECK(hipMemcpyAsync(c, ctl.p, 24, hipMemcpyDeviceToHost, s));
		LQ_HIP_CHECK(hipMemcpyAsync(flags, fl.p, (size_t)nr * 4, hipMemcpyDeviceToHost, s));
		LQ_HIP_CHECK(hipStreamSynchronize(s));
		if (c[2]) LQ_HIP_CHECK(hipMemcpyAsync(items, out.p, (size_t)c[2] * sizeof(PolItem), hipMemcpyDeviceToHost, s));
		LQ_HIP_CHECK(hipStreamSynchronize(s));
		*n_slots = c[2]; *control = (i64)c[0];
	});
}

int lqpol_twin(int kind, const uint8_t *rec, uint64_t len, uint64_t rec_no, uint32_t item[4], int64_t *control, uint32_t *flags, char *errbuf, size_t errbuf_len)
{
	return lq_cabi::guarded(errbuf, errbuf_len, [&] {
		if (!rec || !item || !control || !flags) throw std::invalid_argument("null buffers");
		if (kind != 0 && kind != 1) throw std::invalid_argument("kind is neither 0 (scraps) nor 1 (subreads)");
		if (len < 36 || host_record_len(rec, kind, rec_no) != len) throw std::invalid_argument("not one whole record");
		PolItem it; i64 c;
		*flags = pol_twin(rec, len, kind, rec_no, it, c);
		item[0] = it.zmw; item[1] = it.start; item[2] = it.end; item[3] = it.cls;
		*control = c;
	});
}

} // extern "C"
