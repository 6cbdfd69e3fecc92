// Test-only: longqc_amd/csrc/mmi.hpp (the .mmi format, host only) behind a C ABI, compiled by tests/test_mmi_format.py with g++
// (LQ_EMU: lq_common.hpp without the HIP headers).  Arrays in, arrays out; an exception comes back as -1 with its message.
#define LQ_EMU 1
#include "../../longqc_amd/csrc/mmi.hpp"

namespace {
struct Closer { FILE *f; ~Closer() { if (f) fclose(f); } };
template <class F> int guarded(char *err, size_t errlen, F &&f)
{
	try { return f(); }
	catch (const std::exception &e) { if (err && errlen) snprintf(err, errlen, "%s", e.what()); return -1; }
}
}

// One part written to `path` (appended if `append`): hdr = w, k, b, n_seq, flag; the names back to back with their lengths in
// name_len; the index as mmi_write_index takes it; n_words words of sequence unless the flag says there are none.
extern "C" int shim_mmi_write(const char *path, int append, const uint32_t *hdr, const char *names, const uint32_t *name_len, const uint32_t *lens,
                              uint64_t n_keys, const uint64_t *hkey, const uint64_t *hstart, const uint32_t *hcnt, uint64_t n_pos, const uint64_t *hpos,
                              uint64_t n_words, const uint32_t *words, char *err, size_t errlen)
{
	return guarded(err, errlen, [&] {
		FILE *fp = fopen(path, append ? "ab" : "wb");
		if (!fp) throw std::runtime_error("cannot open the output");
		Closer closer{fp};
		const MmiHeader h{(i32)hdr[0], (i32)hdr[1], hdr[2], hdr[3], hdr[4]};
		std::vector<std::string> nm(h.n_seq);
		for (u32 i = 0; i < h.n_seq; ++i) { nm[i].assign(names, name_len[i]); names += name_len[i]; }
		mmi_write_index(fp, h, nm, std::vector<u32>(lens, lens + h.n_seq), std::vector<u64>(hkey, hkey + n_keys), std::vector<u64>(hstart, hstart + n_keys),
		                std::vector<u32>(hcnt, hcnt + n_keys), std::vector<u64>(hpos, hpos + n_pos));
		if (!(h.flag & LQ_MMI_NO_SEQ)) mmi_write_seq(fp, std::vector<u32>(words, words + n_words));
		return 0;
	});
}

// The part that starts at *offset of `path`, as lqcov_handle::load_part reads it: the header, then the rest.  1: a part, and *offset
// is where it ends; 0: no part there; -1: refused, the message in err.  names: back to back, their lengths in name_len.
extern "C" int shim_mmi_read(const char *path, int64_t *offset, uint32_t *hdr, char *names, size_t names_cap, uint32_t *name_len, uint32_t *lens, uint32_t seq_cap,
                             uint64_t *x, uint64_t *y, uint64_t xy_cap, uint64_t *n_xy, char *err, size_t errlen)
{
	return guarded(err, errlen, [&] {
		FILE *fp = fopen(path, "rb");
		if (!fp) throw std::runtime_error("cannot open the input");
		Closer closer{fp};
		if (fseeko(fp, (off_t)*offset, SEEK_SET) != 0) throw std::runtime_error("cannot seek");
		MmiHeader h;
		if (!mmi_read_header(fp, h)) return 0;
		hdr[0] = (u32)h.w; hdr[1] = (u32)h.k; hdr[2] = h.b; hdr[3] = h.n_seq; hdr[4] = h.flag;
		std::vector<std::string> nm;
		std::vector<u32> ln;
		std::vector<u64> vx, vy;
		mmi_read_part(fp, h, nm, ln, vx, vy);
		size_t name_bytes = 0;
		for (const std::string &s : nm) name_bytes += s.size();
		if (nm.size() > seq_cap || name_bytes > names_cap || vx.size() > xy_cap || vx.size() != vy.size()) throw std::length_error("the test's buffers are too small");
		for (size_t i = 0; i < nm.size(); ++i) { memcpy(names, nm[i].data(), nm[i].size()); names += nm[i].size(); name_len[i] = (u32)nm[i].size(); lens[i] = ln[i]; }
		for (size_t i = 0; i < vx.size(); ++i) { x[i] = vx[i]; y[i] = vy[i]; }
		*n_xy = vx.size();
		*offset = (int64_t)ftello(fp);
		return 1;
	});
}
