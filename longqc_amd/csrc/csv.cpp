// longqc_amd/csrc/csv.cpp -- host side of the delimited-table reader (kernels_csv.hpp) behind the C ABI of include/lqcov.h: lqcsv_*.
// A handle reads the header line itself, uploads the data lines piece by piece -- a piece ends behind a '\n', the line that straddles
// its end is carried into the next -- and keeps one typed column per lqcsv_want on the device.  lqcsv_lengths and the calls behind it
// (the RS-II platform QC's statistics, longqc_amd/rs.py) run on those columns where they lie.
//
// What the device does not answer for goes through csv_twin, this file's own reading of one field, written apart from the kernel's: a
// double outside the device's syntax that is still a number is read by strtod in the C locale, everything else is refused with the line
// and the reason.  Byte offsets that the kernels report become line numbers here, on the host's copy of the piece.
#include "lq_cabi.hpp"
#include "kernels_csv.hpp"
#include "figdata_dev.hpp"
#include "boxstats_dev.hpp"
#include <cerrno>
#include <cmath>
#include <cstdlib>
#include <fcntl.h>
#include <locale.h>
#include <memory>
#include <unistd.h>
#include <vector>

namespace {
constexpr u64 CSV_PAD = 64;
constexpr u64 CSV_PIECE = (u64)8 << 20;

// blocks of a launch: LQ_CSV_MAX_BLOCKS, or fewer with LQCSV_TEST_MAX_BLOCKS (a test hook: the results may not change with it)
u32 max_blocks()
{
	const char *v = getenv("LQCSV_TEST_MAX_BLOCKS");
	const long n = v ? atol(v) : 0;
	return n > 0 && (u64)n < LQ_CSV_MAX_BLOCKS ? (u32)n : LQ_CSV_MAX_BLOCKS;
}
u32 grid_for(u64 items)
{
	const u64 g = (items + LQ_CSV_THREADS - 1) / LQ_CSV_THREADS, cap = max_blocks();
	return (u32)(g < 1 ? 1 : g > cap ? cap : g);
}

u64 count_nl(const u8 *b, u64 from, u64 to)
{
	u64 c = 0;
	for (u64 i = from; i < to; ++i) c += b[i] == '\n';
	return c;
}

bool is_digit(char c) { return c >= '0' && c <= '9'; }

// "[+-]?(digits[.digits?] | .digits)([eE][+-]?digits)?" and nothing else
bool is_number(const std::string &t)
{
	size_t q = 0, d = 0;
	if (q < t.size() && (t[q] == '+' || t[q] == '-')) ++q;
	while (q < t.size() && is_digit(t[q])) { ++q; ++d; }
	if (q < t.size() && t[q] == '.') { ++q; while (q < t.size() && is_digit(t[q])) { ++q; ++d; } }
	if (!d) return false;
	if (q < t.size() && (t[q] == 'e' || t[q] == 'E')) {
		++q;
		if (q < t.size() && (t[q] == '+' || t[q] == '-')) ++q;
		const size_t e0 = q;
		while (q < t.size() && is_digit(t[q])) ++q;
		if (q == e0) return false;
	}
	return q == t.size();
}

// the host twin: one field of a wanted column that k_csv_parse left alone -> its double, or the refusal
double csv_twin(const std::string &t, int kind, const std::string &where)
{
	if (t.empty()) throw std::domain_error(where + "the field is empty");
	if (kind == LQCSV_INT64) {
		size_t q = t[0] == '+' || t[0] == '-' ? 1 : 0, d = 0;
		while (q + d < t.size() && is_digit(t[q + d])) ++d;
		if (d && q + d == t.size()) throw std::domain_error(where + "'" + t + "' has more than 18 digits: it may not fit an int64");
		throw std::domain_error(where + "'" + t + "' is not a whole number");
	}
	if (!is_number(t)) throw std::domain_error(where + "'" + t + "' is not a plain number");
	static const locale_t c_locale = newlocale(LC_ALL_MASK, "C", (locale_t)0);
	if (!c_locale) throw std::logic_error("no C locale");
	const double v = strtod_l(t.c_str(), nullptr, c_locale);
	if (!std::isfinite(v)) throw std::domain_error(where + "'" + t + "' is not a finite double");
	return v;
}
} // namespace

struct lqcsv {
	int device = 0;
	hipStream_t stream = nullptr;
	std::string err;
	int state = 0;                                            // 0: lqcsv_want may come, 1: bytes have come, 2: finished
	u64 piece = CSV_PIECE;
	std::vector<std::string> names; std::vector<int> kinds;
	bool have_header = false;
	CsvWant want;
	u64 line_no = 0;                                          // line breaks consumed so far
	u64 n_rows = 0, cap_rows = 0;
	u64 st_device = 0, st_twin = 0, st_pieces = 0, st_bytes = 0;
	Prim prim;
	DBuf col[LQ_CSV_MAX_WANT];
	DBuf d_bytes, nl, cm, rws, cmb, rowat, rowcm, fbeg, fend, flags, ctl;
	std::vector<u8> h_flags, tail; std::vector<u32> h_beg, h_end;
	// lqcsv_lengths
	bool have_len = false;
	DBuf len_all, hq32, nb32;
	u64 n_mask = 0, n50 = 0, n90 = 0;
	CsvSums sums;

	~lqcsv() { if (stream) (void)hipStreamDestroy(stream); }

	std::string at_line(u64 line) const { return "line " + std::to_string(line) + ": "; }

	void header(const u8 *b, u64 n, u64 line)
	{
		if (n && b[n - 1] == '\r') --n;
		std::vector<std::string> f(1);
		for (u64 i = 0; i < n; ++i) {
			const u8 c = b[i];
			if (c == '"') throw std::domain_error(at_line(line) + "a '\"' in the header: quoted fields are not read");
			if (c == 0) throw std::domain_error(at_line(line) + "a NUL byte in the header");
			if (c == '\r') throw std::domain_error(at_line(line) + "a '\\r' that no '\\n' follows");
			if (c == ',') f.emplace_back(); else f.back().push_back((char)c);
		}
		want.n = (u32)names.size(); want.n_fields = (u32)f.size();
		for (size_t k = 0; k < names.size(); ++k) {
			size_t j = 0;
			while (j < f.size() && f[j] != names[k]) ++j;          // (of a repeated name the first column)
			if (j == f.size()) throw std::domain_error(at_line(line) + "the header has no column '" + names[k] + "'");
			want.field[k] = (u32)j; want.kind[k] = (u32)kinds[k]; want.out[k] = nullptr;
		}
		have_header = true;
	}

	void rows_room(u64 more)
	{
		if (n_rows + more >= (1ULL << 32) - 1) throw std::domain_error("2^32 rows or more");
		if (n_rows + more <= cap_rows) return;
		const u64 cap = std::max(n_rows + more, 2 * cap_rows);
		for (u32 k = 0; k < want.n; ++k) col[k].grow((size_t)cap * 8, (size_t)cap * 8, (size_t)n_rows * 8, stream);      // (room for cap_rows, not for this piece alone)
		cap_rows = cap;
	}

	// h[0 .. n): whole data lines, each ending in '\n'; line0: the line breaks in front of h[0]
	void device_piece(const u8 *h, u64 n, u64 line0)
	{
		if (n >= LQ_CSV_MAX_BYTES) throw std::domain_error("a piece of 2^32 bytes or more");
		const auto line_of = [&](u64 at) { return line0 + count_nl(h, 0, at) + 1; };
		d_bytes.ensure((size_t)(n + CSV_PAD));
		nl.ensure((size_t)(n + 1) * 4); cm.ensure((size_t)(n + 1) * 4); rws.ensure((size_t)(n + 1) * 4); cmb.ensure((size_t)(n + 1) * 4); ctl.ensure(32);
		const unsigned long long init[4] = { LQ_CSV_NONE, LQ_CSV_NONE, 0, 0 };
		LQ_HIP_CHECK(hipMemcpyAsync(d_bytes.p, h, (size_t)n, hipMemcpyHostToDevice, stream));
		LQ_HIP_CHECK(hipMemsetAsync(d_bytes.as<u8>() + n, 0, CSV_PAD, stream));
		LQ_HIP_CHECK(hipMemcpyAsync(ctl.p, init, 32, hipMemcpyHostToDevice, stream));
		const u8 *d = d_bytes.as<u8>();
		unsigned long long *c = ctl.as<unsigned long long>();
		LQ_LAUNCH(k_csv_marks, grid_for(n + 1), LQ_CSV_THREADS, stream, d, n, nl.as<u32>(), cm.as<u32>(), c);
		LQ_HIP_CHECK(hipGetLastError());
		prim.exclusive_scan_u32_u32(nl.as<u32>(), rws.as<u32>(), (size_t)n + 1);
		prim.exclusive_scan_u32_u32(cm.as<u32>(), cmb.as<u32>(), (size_t)n + 1);
		unsigned long long got[4];
		u32 rows = 0;
		LQ_HIP_CHECK(hipMemcpyAsync(got, ctl.p, 32, hipMemcpyDeviceToHost, stream));
		LQ_HIP_CHECK(hipMemcpyAsync(&rows, rws.as<u32>() + n, 4, hipMemcpyDeviceToHost, stream));
		LQ_HIP_CHECK(hipStreamSynchronize(stream));
		if (got[0] != LQ_CSV_NONE) {
			const u64 at = got[0];
			if (at >= n) throw std::logic_error("the offending byte lies outside the piece");
			const u8 ch = h[at];
			throw std::domain_error(at_line(line_of(at)) + (ch == '"' ? "a '\"': quoted fields are not read" : ch == 0 ? "a NUL byte" : "a '\\r' that no '\\n' follows"));
		}
		if (!rows) return;
		const u32 nw = want.n;
		const u64 n_pairs = (u64)rows * nw;
		rowat.ensure((size_t)rows * 4); rowcm.ensure((size_t)rows * 4);
		fbeg.ensure((size_t)std::max<u64>(n_pairs, 1) * 4); fend.ensure((size_t)std::max<u64>(n_pairs, 1) * 4); flags.ensure((size_t)std::max<u64>(n_pairs, 1));
		if (n_pairs) {                                             // (a ragged row leaves entries unwritten: never a stale position)
			LQ_HIP_CHECK(hipMemsetAsync(fbeg.p, 0xff, (size_t)n_pairs * 4, stream));
			LQ_HIP_CHECK(hipMemsetAsync(fend.p, 0, (size_t)n_pairs * 4, stream));
		}
		LQ_LAUNCH(k_csv_rows, grid_for(n), LQ_CSV_THREADS, stream, d, n, (const u32*)rws.as<u32>(), (const u32*)cmb.as<u32>(), rows, rowat.as<u32>(), rowcm.as<u32>());
		LQ_LAUNCH(k_csv_starts, grid_for(n), LQ_CSV_THREADS, stream, d, n, (const u32*)rws.as<u32>(), (const u32*)cmb.as<u32>(), (const u32*)rowat.as<u32>(), (const u32*)rowcm.as<u32>(), rows, want,
		          fbeg.as<u32>(), fend.as<u32>(), c);
		LQ_HIP_CHECK(hipGetLastError());
		LQ_HIP_CHECK(hipMemcpyAsync(got, ctl.p, 32, hipMemcpyDeviceToHost, stream));
		LQ_HIP_CHECK(hipStreamSynchronize(stream));
		if (got[1] != LQ_CSV_NONE) {
			const u64 at = got[1];
			if (at >= n) throw std::logic_error("the ragged row lies outside the piece");
			u64 e = at, fields = 1;
			while (e < n && h[e] != '\n') fields += h[e++] == ',';
			throw std::domain_error(at_line(line_of(at)) + "the row has " + std::to_string(fields) + " fields, the header has " + std::to_string(want.n_fields));
		}
		if (n_pairs) {
			rows_room(rows);
			for (u32 k = 0; k < nw; ++k) want.out[k] = col[k].p;
			LQ_LAUNCH(k_csv_parse, grid_for(n_pairs), LQ_CSV_THREADS, stream, d, n, (const u32*)fbeg.as<u32>(), (const u32*)fend.as<u32>(), rows, want, n_rows, flags.as<u8>(), c);
			LQ_HIP_CHECK(hipGetLastError());
			LQ_HIP_CHECK(hipMemcpyAsync(got, ctl.p, 32, hipMemcpyDeviceToHost, stream));
			LQ_HIP_CHECK(hipStreamSynchronize(stream));
			const u64 n_host = got[2];
			if (n_host) {                                         // the twin reads the flagged fields, in file order
				h_flags.resize((size_t)n_pairs); h_beg.resize((size_t)n_pairs); h_end.resize((size_t)n_pairs);
				LQ_HIP_CHECK(hipMemcpyAsync(h_flags.data(), flags.p, (size_t)n_pairs, hipMemcpyDeviceToHost, stream));
				LQ_HIP_CHECK(hipMemcpyAsync(h_beg.data(), fbeg.p, (size_t)n_pairs * 4, hipMemcpyDeviceToHost, stream));
				LQ_HIP_CHECK(hipMemcpyAsync(h_end.data(), fend.p, (size_t)n_pairs * 4, hipMemcpyDeviceToHost, stream));
				LQ_HIP_CHECK(hipStreamSynchronize(stream));
				// (the rows ascend in the piece, so the line count goes on from the field before; a field in front of `seen` lies in its row)
				u64 seen = 0, lines = 0;
				std::vector<double> fixed;
				std::vector<double*> dst;
				for (u64 r = 0; r < rows; ++r)
					for (u32 k = 0; k < nw; ++k) {
						const u64 p = r * nw + k;
						if (!h_flags[p]) continue;
						const u64 b = h_beg[p], e = h_end[p];
						if (b > e || e > n) throw std::logic_error("a flagged field lies outside the piece");
						if (b >= seen) { lines += count_nl(h, seen, b); seen = b; }
						const std::string where = at_line(line0 + lines + 1) + "column '" + names[k] + "': ";
						fixed.push_back(csv_twin(std::string((const char*)h + b, (size_t)(e - b)), kinds[k], where));
						dst.push_back(col[k].as<double>() + n_rows + r);
					}
				for (size_t i = 0; i < fixed.size(); ++i) LQ_HIP_CHECK(hipMemcpyAsync(dst[i], &fixed[i], 8, hipMemcpyHostToDevice, stream));
				LQ_HIP_CHECK(hipStreamSynchronize(stream));
				st_twin += fixed.size();
			}
			st_device += n_pairs - n_host;
		}
		n_rows += rows;
	}

	// h[0 .. n): whole lines
	void lines(const u8 *h, u64 n)
	{
		++st_pieces; st_bytes += n;
		u64 at = 0;
		if (!have_header) {
			while (at < n && (h[at] == '\n' || (h[at] == '\r' && at + 1 < n && h[at + 1] == '\n'))) at += h[at] == '\n' ? 1 : 2;
			if (at < n) {
				const u8 *e = (const u8*)memchr(h + at, '\n', (size_t)(n - at));
				const u64 end = (u64)(e - h);
				header(h + at, end - at, line_no + count_nl(h, 0, at) + 1);
				at = end + 1;
			}
		}
		if (at < n) device_piece(h + at, n - at, line_no + count_nl(h, 0, at));
		line_no += count_nl(h, 0, n);
	}

	// -> the bytes consumed
	u64 feed(const u8 *b, u64 n, bool last)
	{
		if (state == 2) throw std::logic_error("the handle is finished");
		state = 1;
		u64 pos = 0;
		while (pos < n) {
			u64 lim = std::min(n, pos + piece);
			const void *e = memrchr(b + pos, '\n', (size_t)(lim - pos));
			while (!e && lim < n) {                                // a line longer than a piece
				const u64 from = lim;
				lim = std::min(n, lim + piece);
				e = memchr(b + from, '\n', (size_t)(lim - from));
			}
			if (e) {
				const u64 end = (u64)((const u8*)e - b) + 1;
				lines(b + pos, end - pos);
				pos = end;
			} else if (last) {                                     // the last line has no line break: it is a row all the same
				tail.assign(b + pos, b + n);
				tail.push_back('\n');
				lines(tail.data(), tail.size());
				--st_bytes;
				pos = n;
			} else break;
		}
		return pos;
	}

	void add_file(const std::string &path)
	{
		struct Fd { int fd = -1; ~Fd() { if (fd >= 0) ::close(fd); } } f;
		f.fd = ::open(path.c_str(), O_RDONLY);
		if (f.fd < 0) throw lq_open_error(path);
		std::vector<u8> buf;
		u64 fill = 0;
		bool ended = false;
		try {
			while (!ended) {
				if (buf.size() < fill + piece) buf.resize((size_t)(fill + piece));
				const u64 room = buf.size() - fill;
				u64 got = 0;
				while (got < room) {
					const ssize_t r = ::read(f.fd, buf.data() + fill + got, (size_t)(room - got));
					if (r < 0) { if (errno == EINTR) continue; throw lq_open_error(path, "read error"); }
					if (r == 0) { ended = true; break; }
					got += (u64)r;
				}
				fill += got;
				const u64 used = feed(buf.data(), fill, ended);
				if (used) memmove(buf.data(), buf.data() + used, (size_t)(fill - used));
				fill -= used;
			}
		} catch (const std::domain_error &e) { throw std::domain_error(path + ": " + e.what()); }
	}

	void need_finished() const { if (state != 2) throw std::logic_error("lqcsv_finish has not been called"); }
	void need_lengths() const { need_finished(); if (!have_len) throw std::logic_error("lqcsv_lengths has not been called"); }
	u32 col_of(u32 c, int kind, const char *what) const
	{
		if (c >= names.size()) throw std::invalid_argument(std::string(what) + ": no such column");
		if (kinds[c] != kind) throw std::invalid_argument(std::string(what) + ": column '" + names[c] + "' is not of kind " + (kind == LQCSV_INT64 ? "int64" : "double"));
		return c;
	}

	void lengths(u32 score_col, double threshold, u32 start_col, u32 end_col, u32 bases_col, u64 *out)
	{
		need_finished();
		col_of(score_col, LQCSV_DOUBLE, "score_col"); col_of(start_col, LQCSV_INT64, "start_col"); col_of(end_col, LQCSV_INT64, "end_col"); col_of(bases_col, LQCSV_INT64, "bases_col");
		if (threshold != threshold) throw std::invalid_argument("the threshold is NaN");
		have_len = false; n_mask = n50 = n90 = 0;
		const CsvSums init = { 0, ~0ULL, 0, 0, ~0ULL, 0, 0 };
		sums = init;
		for (u32 k = 0; k < LQCSV_LEN_WORDS; ++k) out[k] = 0;
		const u64 n = n_rows;
		if (!n) { have_len = true; return; }
		DBuf flag, pos, key, key_s, v, ex, d_sums, d_pol;
		len_all.ensure((size_t)n * 4); flag.ensure((size_t)(n + 1) * 4); pos.ensure((size_t)(n + 1) * 4); d_sums.ensure(sizeof(CsvSums));
		LQ_HIP_CHECK(hipMemcpyAsync(d_sums.p, &init, sizeof(CsvSums), hipMemcpyHostToDevice, stream));
		LQ_LAUNCH(k_csv_lengths, grid_for(n + 1), LQ_CSV_THREADS, stream, (const i64*)col[start_col].as<i64>(), (const i64*)col[end_col].as<i64>(), (const double*)col[score_col].as<double>(), threshold, n,
		          len_all.as<u32>(), flag.as<u32>(), &d_sums.as<CsvSums>()->n_range);
		LQ_HIP_CHECK(hipGetLastError());
		prim.exclusive_scan_u32_u32(flag.as<u32>(), pos.as<u32>(), (size_t)n + 1);
		u32 m = 0;
		CsvSums first;
		LQ_HIP_CHECK(hipMemcpyAsync(&m, pos.as<u32>() + n, 4, hipMemcpyDeviceToHost, stream));
		LQ_HIP_CHECK(hipMemcpyAsync(&first, d_sums.p, sizeof(CsvSums), hipMemcpyDeviceToHost, stream));
		LQ_HIP_CHECK(hipStreamSynchronize(stream));
		if (first.n_range) throw std::domain_error(std::to_string(first.n_range) + " rows whose '" + names[end_col] + "' - '" + names[start_col] + "' lies below 0 or above 2^32-1");
		n_mask = m;
		if (m) {
			hq32.ensure((size_t)m * 4); nb32.ensure((size_t)m * 4); key.ensure((size_t)m * 4); key_s.ensure((size_t)m * 4); v.ensure((size_t)m * 4); ex.ensure((size_t)m * 8);
			d_pol.ensure(sizeof(PolSums));
			LQ_LAUNCH(k_csv_pack, grid_for(n), LQ_CSV_THREADS, stream, (const u32*)len_all.as<u32>(), (const i64*)col[bases_col].as<i64>(), (const u32*)flag.as<u32>(), (const u32*)pos.as<u32>(), n,
			          hq32.as<u32>(), nb32.as<u32>(), key.as<u32>(), d_sums.as<CsvSums>());
			LQ_HIP_CHECK(hipGetLastError());
			LQ_HIP_CHECK(hipMemcpyAsync(&sums, d_sums.p, sizeof(CsvSums), hipMemcpyDeviceToHost, stream));
			LQ_HIP_CHECK(hipStreamSynchronize(stream));
			if (sums.n_range) throw std::domain_error(std::to_string(sums.n_range) + " rows under the mask whose '" + names[bases_col] + "' lies below 0 or above 2^32-1");
			if (sums.sum_hq >= (1ULL << 53) / 100) throw std::domain_error("100 times the throughput reaches 2^53: N50 and N90 by integers would no longer be the reference's");
			// N50 / N90 as polread.cpp takes them: the descending sort, the scan, k_pol_nxx on a PolSums that holds the sum
			PolSums ps = {0, 0, ~0ULL, 0, 0, 0, 0xffffffffu, 0, 0, 0};
			ps.sum_hq = sums.sum_hq;
			LQ_HIP_CHECK(hipMemcpyAsync(d_pol.p, &ps, sizeof(PolSums), hipMemcpyHostToDevice, stream));
			prim.sort_keys_u32(key.as<u32>(), key_s.as<u32>(), (size_t)m);
			LQ_LAUNCH(k_pol_unkey, grid_for(m), LQ_CSV_THREADS, stream, (const u32*)key_s.as<u32>(), (u64)m, v.as<u32>());
			LQ_HIP_CHECK(hipGetLastError());
			prim.exclusive_scan_u32_u64(v.as<u32>(), ex.as<u64>(), (size_t)m);
			LQ_LAUNCH(k_pol_nxx, grid_for(m), LQ_CSV_THREADS, stream, (const u32*)v.as<u32>(), (const u64*)ex.as<u64>(), (u64)m, d_pol.as<PolSums>());
			LQ_HIP_CHECK(hipGetLastError());
			LQ_HIP_CHECK(hipMemcpyAsync(&ps, d_pol.p, sizeof(PolSums), hipMemcpyDeviceToHost, stream));
			LQ_HIP_CHECK(hipStreamSynchronize(stream));
			n50 = ps.n50; n90 = ps.n90;
			const u64 w[LQCSV_LEN_WORDS] = { n_mask, sums.sum_hq, sums.min_hq, sums.max_hq, n50, n90, sums.sum_nb, sums.min_nb, sums.max_nb, 0 };
			memcpy(out, w, sizeof(w));
		}
		have_len = true;
	}

	const DBuf &array(int which, u64 *n) const
	{
		need_lengths();
		if (which != LQCSV_HQ && which != LQCSV_BASES && which != LQCSV_LEN_ALL) throw std::invalid_argument("which is none of LQCSV_HQ, LQCSV_BASES, LQCSV_LEN_ALL");
		*n = which == LQCSV_LEN_ALL ? n_rows : n_mask;
		return which == LQCSV_HQ ? hq32 : which == LQCSV_BASES ? nb32 : len_all;
	}
};

namespace {
static_assert(LQ_CSV_THREADS == LQ_POL_THREADS, "k_pol_unkey and k_pol_nxx stride by LQ_POL_THREADS");

template <class F> int csv_call(lqcsv *p, F &&f)
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
thread_local std::string g_csv_error;
} // namespace

extern "C" {

lqcsv *lqcsv_create(int device)
{
	try {
		lq_cabi::select_device(device);
		std::unique_ptr<lqcsv> p(new lqcsv());
		p->device = device;
		LQ_HIP_CHECK(hipStreamCreate(&p->stream));
		p->prim.stream = p->stream;
		p->want.n = p->want.n_fields = 0;
		return p.release();
	} catch (const std::exception &e) { g_csv_error = e.what(); return nullptr; }
}

void lqcsv_destroy(lqcsv *p) { delete p; }

const char *lqcsv_last_error(const lqcsv *p) { return p ? p->err.c_str() : g_csv_error.c_str(); }

int lqcsv_want(lqcsv *p, const char *name, int kind)
{
	return csv_call(p, [&] {
		if (!name) throw std::invalid_argument("null name");
		if (kind != LQCSV_INT64 && kind != LQCSV_DOUBLE) throw std::invalid_argument("kind is neither LQCSV_INT64 nor LQCSV_DOUBLE");
		if (p->state != 0) throw std::logic_error("lqcsv_want after bytes have arrived");
		if (p->names.size() == LQ_CSV_MAX_WANT) throw std::invalid_argument("more than 16 wanted columns");
		for (const std::string &s : p->names) if (s == name) throw std::invalid_argument("the column '" + s + "' is wanted already");
		p->names.push_back(name); p->kinds.push_back(kind);
	});
}

int lqcsv_set_piece_bytes(lqcsv *p, uint64_t bytes)
{
	return csv_call(p, [&] {
		if (bytes >= LQ_CSV_MAX_BYTES / 2) throw std::invalid_argument("a piece of 2^31 bytes or more");
		p->piece = bytes ? bytes : CSV_PIECE;
	});
}

int lqcsv_add_bytes(lqcsv *p, const uint8_t *bytes, uint64_t n, int last, uint64_t *resume)
{
	return csv_call(p, [&] {
		if (!resume || (n && !bytes)) throw std::invalid_argument("null buffers");
		*resume = 0;
		*resume = p->feed(bytes, n, last != 0);
	});
}

int lqcsv_add_file(lqcsv *p, const char *path)
{
	return csv_call(p, [&] {
		if (!path) throw std::invalid_argument("null path");
		if (p->state == 2) throw std::logic_error("the handle is finished");
		p->add_file(path);
	});
}

int lqcsv_finish(lqcsv *p, uint64_t *n_rows)
{
	return csv_call(p, [&] {
		if (!n_rows) throw std::invalid_argument("null buffers");
		if (p->state == 2) throw std::logic_error("the handle is finished");
		if (!p->have_header) throw std::domain_error("line 1: no header line: the table is empty");
		p->state = 2;
		*n_rows = p->n_rows;
	});
}

int lqcsv_get(lqcsv *p, uint32_t col, void *out)
{
	return csv_call(p, [&] {
		p->need_finished();
		if (col >= p->names.size()) throw std::invalid_argument("no such column");
		if (!p->n_rows) return;
		if (!out) throw std::invalid_argument("null buffers");
		LQ_HIP_CHECK(hipMemcpyAsync(out, p->col[col].p, (size_t)p->n_rows * 8, hipMemcpyDeviceToHost, p->stream));
		LQ_HIP_CHECK(hipStreamSynchronize(p->stream));
	});
}

int lqcsv_stats(const lqcsv *p, uint64_t out[LQCSV_STATS_WORDS])
{
	if (!p || !out) return LQCOV_E_ARG;
	const uint64_t v[LQCSV_STATS_WORDS] = { p->n_rows, p->st_device, p->st_twin, p->st_pieces, p->st_bytes };
	memcpy(out, v, sizeof(v));
	return 0;
}

int lqcsv_lengths(lqcsv *p, uint32_t score_col, double threshold, uint32_t start_col, uint32_t end_col, uint32_t bases_col,
                  uint64_t out[LQCSV_LEN_WORDS])
{
	return csv_call(p, [&] {
		if (!out) throw std::invalid_argument("null buffers");
		p->lengths(score_col, threshold, start_col, end_col, bases_col, out);
	});
}

int lqcsv_get_lengths(lqcsv *p, int which, uint32_t *out)
{
	return csv_call(p, [&] {
		u64 n = 0;
		const DBuf &x = p->array(which, &n);
		if (!n) return;
		if (!out) throw std::invalid_argument("null buffers");
		LQ_HIP_CHECK(hipMemcpyAsync(out, x.p, (size_t)n * 4, hipMemcpyDeviceToHost, p->stream));
		LQ_HIP_CHECK(hipStreamSynchronize(p->stream));
	});
}

int lqcsv_hist(lqcsv *p, int which, const double *edges, uint32_t n_edges, uint64_t *counts)
{
	return csv_call(p, [&] {
		u64 n = 0;
		const DBuf &x = p->array(which, &n);
		if (n_edges && !edges) throw std::invalid_argument("null buffers");
		for (u32 k = 0; k < n_edges; ++k)
			if (edges[k] != edges[k] || (k && edges[k] < edges[k - 1])) throw std::invalid_argument("edges are not ascending");
		if (n_edges < 2) return;
		if (!counts) throw std::invalid_argument("null buffers");
		for (u32 k = 0; k + 1 < n_edges; ++k) counts[k] = 0;
		if (!n) return;
		lq_fig_hist_dev(p->stream, LQFIG_U32, x.p, n, edges, n_edges, counts);
	});
}

int lqcsv_logsum(lqcsv *p, uint64_t *sum, double *sum_log, uint64_t *n_zero)
{
	return csv_call(p, [&] {
		p->need_lengths();
		if (!sum || !sum_log || !n_zero) throw std::invalid_argument("null buffers");
		*sum = 0; *sum_log = 0.0; *n_zero = 0;
		if (!p->n_mask) return;
		lq_fig_logsum_dev(p->stream, p->hq32.as<u32>(), p->n_mask, sum, sum_log, n_zero);
	});
}

int lqcsv_boxstats(lqcsv *p, uint32_t value_col, double interval, double whis, double *sorted, lqfig_box_f64 *boxes, uint32_t box_cap,
                   uint32_t *n_boxes)
{
	return csv_call(p, [&] {
		if (!n_boxes) throw std::invalid_argument("null buffers");
		*n_boxes = 0;
		p->need_lengths();
		p->col_of(value_col, LQCSV_DOUBLE, "value_col");
		lq_box_f64_dev(p->stream, p->len_all.as<u32>(), p->col[value_col].as<double>(), p->n_rows, interval, whis, sorted, boxes, box_cap, n_boxes);
	});
}

} // extern "C"
