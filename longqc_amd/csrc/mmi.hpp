// longqc_amd/csrc/mmi.hpp -- the reference's index files (.mmi; mm_idx_dump / mm_idx_load, index.c:385-540) as bytes: the format
// alone, host only.  No device call and no handle: lqcov_handle::dump_part / load_part (engine.cpp) bring a part's arrays to the host
// and back, run_files (runfiles.cpp) probes its target with the same header reader.
//
// One part in the reference's on-disk layout.  What a reader needs is reproduced exactly (header, names with their
// one-byte length, per-bucket position arrays with every list ascending, key = minimizer>>b<<1 | singleton, value = the
// position or start<<32 | n, 4-bit sequences); the order of the (key, value) pairs inside a bucket is ascending key here,
// khash slot order in the reference -- mm_idx_load re-inserts them one by one, so the order is immaterial.
#pragma once
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>
#include <sys/types.h>
#include "lq_common.hpp"

#define LQ_MMI_MAGIC "MMI\2"
#define LQ_MMI_BUCKET_BITS 14           // mm_idxopt_init (index.c:33); the option table has no switch for it
#define LQ_MMI_NO_SEQ 0x2

struct MmiHeader { i32 w, k; u32 b, n_seq, flag; };   // in the file's order; flag: bit 0 -H, LQ_MMI_NO_SEQ

static inline void fwrite_or_throw(const void *p, size_t sz, size_t n, FILE *fp)
{
	if (n && fwrite(p, sz, n, fp) != n) throw std::runtime_error("write to the index dump failed");
}

static inline bool fread_exact(void *p, size_t sz, size_t n, FILE *fp) { return n == 0 || fread(p, sz, n, fp) == n; }

// The magic and the header of the part that starts here.  false: no part -- the end of the file (index.c:436) or other bytes than the
// magic (mm_idx_is_idx, index.c:481-498).
static inline bool mmi_read_header(FILE *fp, MmiHeader &h)
{
	char magic[4];
	if (fread(magic, 1, 4, fp) != 4) return false;
	if (memcmp(magic, LQ_MMI_MAGIC, 4) != 0) return false;
	u32 hdr[5];
	if (!fread_exact(hdr, 4, 5, fp)) throw std::runtime_error("truncated index file");
	h.w = (i32)hdr[0]; h.k = (i32)hdr[1]; h.b = hdr[2]; h.n_seq = hdr[3]; h.flag = hdr[4];
	return true;
}

// What follows the header, up to the next part: the sequences' names and lengths, and every minimizer of the index with its
// positions, x = minimizer << 8 and y = the position as the index holds it, bucket by bucket.
static inline void mmi_read_part(FILE *fp, const MmiHeader &h, std::vector<std::string> &names, std::vector<u32> &lens, std::vector<u64> &x, std::vector<u64> &y)
{
	const u32 b = h.b;
	if (b > 30) throw std::runtime_error("corrupt index file (bucket bits)");
	names.assign(h.n_seq, std::string()); lens.assign(h.n_seq, 0);
	x.clear(); y.clear();
	u64 sum_len = 0;
	for (u32 i = 0; i < h.n_seq; ++i) {
		u8 l;
		char buf[256];
		if (!fread_exact(&l, 1, 1, fp) || !fread_exact(buf, 1, l, fp) || !fread_exact(&lens[i], 4, 1, fp)) throw std::runtime_error("truncated index file");
		names[i].assign(buf, strnlen(buf, l));                     // the reference holds it as a C string (index.c:448-450)
		sum_len += lens[i];
	}
	std::vector<u64> pbuf;
	for (u32 bi = 0; bi < (1u << b); ++bi) {
		i32 n_p; u32 size;
		if (!fread_exact(&n_p, 4, 1, fp) || n_p < 0) throw std::runtime_error("truncated index file");
		pbuf.resize((size_t)n_p);
		if (!fread_exact(pbuf.data(), 8, (size_t)n_p, fp) || !fread_exact(&size, 4, 1, fp)) throw std::runtime_error("truncated index file");
		for (u32 j = 0; j < size; ++j) {
			u64 kv[2];
			if (!fread_exact(kv, 8, 2, fp)) throw std::runtime_error("truncated index file");
			const u64 minier = (kv[0] >> 1) << b | bi;             // index.c:69-86 read backwards
			if (kv[0] & 1) { x.push_back(minier << 8); y.push_back(kv[1]); }
			else {
				const u64 st = kv[1] >> 32, n = (u32)kv[1];
				if (st + n > (u64)n_p) throw std::runtime_error("corrupt index file (position list)");
				for (u64 t = 0; t < n; ++t) { x.push_back(minier << 8); y.push_back(pbuf[st + t]); }
			}
		}
	}
	if (!(h.flag & LQ_MMI_NO_SEQ)) {                              // mi->S: not used on this path; skipped
		const u64 bytes = (sum_len + 7) / 8 * 4;
		if (fseeko(fp, (off_t)bytes, SEEK_CUR) != 0) throw std::runtime_error("truncated index file");
	}
}

// Magic, header, names and buckets of one part.  The index as the build leaves it: the distinct minimizers ascending (hkey), and for
// each where its positions start in hpos and how many there are.
static inline void mmi_write_index(FILE *fp, const MmiHeader &h, const std::vector<std::string> &names, const std::vector<u32> &lens,
                                   const std::vector<u64> &hkey, const std::vector<u64> &hstart, const std::vector<u32> &hcnt, const std::vector<u64> &hpos)
{
	const u64 K = hkey.size();
	const u32 b = h.b, nb = 1u << b;
	const u32 hdr[5] = {(u32)h.w, (u32)h.k, b, h.n_seq, h.flag};
	fwrite_or_throw(LQ_MMI_MAGIC, 1, 4, fp);
	fwrite_or_throw(hdr, 4, 5, fp);
	for (u32 i = 0; i < h.n_seq; ++i) {
		const u8 l = (u8)names[i].size();                          // index.c:401: the length is stored in one byte
		fwrite_or_throw(&l, 1, 1, fp);
		fwrite_or_throw(names[i].data(), 1, l, fp);
		fwrite_or_throw(&lens[i], 4, 1, fp);
	}
	// keys by bucket (low b bits); hkey is ascending, so every bucket's keys stay ascending
	std::vector<u64> bstart(nb + 1, 0);
	for (u64 i = 0; i < K; ++i) ++bstart[(hkey[i] & (nb - 1)) + 1];
	for (u32 i = 0; i < nb; ++i) bstart[i + 1] += bstart[i];
	std::vector<u64> order(K), fill(bstart.begin(), bstart.end() - 1);
	for (u64 i = 0; i < K; ++i) order[fill[hkey[i] & (nb - 1)]++] = i;
	std::vector<u64> pbuf, kv;
	for (u32 bi = 0; bi < nb; ++bi) {
		pbuf.clear(); kv.clear();
		for (u64 t = bstart[bi]; t < bstart[bi + 1]; ++t) {
			const u64 i = order[t];
			const u64 key = hkey[i] >> b << 1;
			if (hcnt[i] == 1) { kv.push_back(key | 1); kv.push_back(hpos[hstart[i]]); }
			else {
				kv.push_back(key); kv.push_back((u64)pbuf.size() << 32 | hcnt[i]);
				pbuf.insert(pbuf.end(), hpos.begin() + hstart[i], hpos.begin() + hstart[i] + hcnt[i]);
			}
		}
		if (pbuf.size() > 0x7fffffffULL) throw std::domain_error("index bucket too large for the .mmi format");
		const i32 n_p = (i32)pbuf.size();
		const u32 size = (u32)(kv.size() / 2);
		fwrite_or_throw(&n_p, 4, 1, fp);
		fwrite_or_throw(pbuf.data(), 8, pbuf.size(), fp);
		fwrite_or_throw(&size, 4, 1, fp);
		fwrite_or_throw(kv.data(), 8, kv.size(), fp);
	}
}

// mi->S: the part's sequences end to end, 4 bits a base, eight bases a word (k_seq4 packs them)
static inline void mmi_write_seq(FILE *fp, const std::vector<u32> &words) { fwrite_or_throw(words.data(), 4, words.size(), fp); }
