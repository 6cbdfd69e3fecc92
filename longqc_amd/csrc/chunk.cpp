// longqc_amd/csrc/chunk.cpp -- the resident chunk and the packed store behind the C ABI of include/lqcov.h (lqchunk_*, lqstore_*):
// what makes the per-chunk steps of sampleqc and the coverage engine one pass over the input.  A chunk's bases go to the device
// once (lq_chunk_ready); the low-complexity scan, the adapter search and the GC counts run on them (dust.cpp, adapt.cpp, gc.cpp);
// k_chunk_pack (kernels_chunk.hpp) turns them into the engine's packed layout there; the store keeps the packed chunks in device
// memory and, when every chunk has been seen, hands them to the engine part by part (lqcov_part_add_packed_shares_dev): the
// input is neither read nor uploaded a second time (the reference parses its input file twice, minimap2-coverage.c:273,408).
#include "engine.hpp"
#include "chunk.hpp"
#include "kernels_chunk.hpp"
#include "kernels_gather.hpp"
#include "kernels_bam.hpp"
#include "kernels_fxscan.hpp"
#include <algorithm>
#include <memory>

void lq_chunk_set(lqchunk &c, u32 n, const u8 *seq, const u64 *seq_off, const u8 *qual)
{
	c.n = n; c.first_desc = n;
	c.off.resize((size_t)n + 1);
	for (u32 i = 0; i <= n; ++i) c.off[i] = seq_off[i] - seq_off[0];
	for (u32 i = 0; i < n; ++i) if (seq_off[i + 1] < seq_off[i]) { c.first_desc = i; break; }
	c.total = c.off[n];
	c.h_seq = seq ? seq + seq_off[0] : nullptr;
	c.h_qual = qual ? qual + seq_off[0] : nullptr;
	c.has_qual = qual != nullptr;
	c.resident = false; c.packed = false; c.n_chunks = 0; c.iv_valid = false; c.dust_done = false; c.cols_done = false;
}

void lq_chunk_ready(lqchunk &c)
{
	lq_cabi::select_device(c.device);
	if (!c.stream) LQ_HIP_CHECK(hipStreamCreate(&c.stream));
	if (c.resident) return;
	// whole tiles of k_gc_reads and LQ_PACK_PAD bytes behind the last base (k_chunk_pack's third load, k_sdust's and k_gc_windows' 16), zeroed
	const u64 alloc = (c.total + LQ_CHUNK_SEQ_TILE - 1) / LQ_CHUNK_SEQ_TILE * LQ_CHUNK_SEQ_TILE + LQ_PACK_PAD;
	c.seq.ensure((size_t)alloc);
	if (c.total) LQ_HIP_CHECK(hipMemcpyAsync(c.seq.p, c.h_seq, (size_t)c.total, hipMemcpyHostToDevice, c.stream));
	LQ_HIP_CHECK(hipMemsetAsync(c.seq.as<u8>() + c.total, 0, (size_t)(alloc - c.total), c.stream));
	c.d_off.ensure(((size_t)c.n + 1) * 8);
	LQ_HIP_CHECK(hipMemcpyAsync(c.d_off.p, c.off.data(), ((size_t)c.n + 1) * 8, hipMemcpyHostToDevice, c.stream));
	if (c.has_qual) {
		c.qual.ensure((size_t)c.total + LQ_GATHER_SRC_PAD);       // (k_fastq_format's second load)
		if (c.total) LQ_HIP_CHECK(hipMemcpyAsync(c.qual.p, c.h_qual, (size_t)c.total, hipMemcpyHostToDevice, c.stream));
	}
	LQ_HIP_CHECK(hipStreamSynchronize(c.stream));             // the caller's buffers are free again
	c.h_seq = c.h_qual = nullptr;
	c.resident = true;
}

// kind: 0 bytes (k_chunk_gather), 1 a BAM file's packed sequences (k_bam_gather), 2 its quality bytes (k_bam_qual)
static void gather_launch(lqchunk &c, const u8 *raw, std::vector<GatherSeg> &segs, u8 *dst, bool upper, int kind)
{
	const u64 total = c.total;
	if (!total) return;
	const u64 n_segs = segs.size(), n_tiles = (total + LQ_GATHER_TILE - 1) / LQ_GATHER_TILE;
	if (n_segs > 0xffffffffULL) throw std::domain_error("more than 2^32-1 lines in one chunk");
	segs.push_back({0, total});
	std::vector<u32> tile_seg((size_t)n_tiles + 1);           // the work list: the segment that holds the first byte of every tile
	{
		u64 s = 0;
		for (u64 t = 0; t < n_tiles; ++t) {
			while (s + 1 < n_segs && segs[s + 1].dst <= t * LQ_GATHER_TILE) ++s;
			tile_seg[t] = (u32)s;
		}
		tile_seg[n_tiles] = (u32)(n_segs - 1);
	}
	c.gseg.ensure((n_segs + 1) * sizeof(GatherSeg)); c.gtile.ensure((n_tiles + 1) * 4);
	LQ_HIP_CHECK(hipMemcpyAsync(c.gseg.p, segs.data(), (n_segs + 1) * sizeof(GatherSeg), hipMemcpyHostToDevice, c.stream));
	LQ_HIP_CHECK(hipMemcpyAsync(c.gtile.p, tile_seg.data(), (n_tiles + 1) * 4, hipMemcpyHostToDevice, c.stream));
	const u32 grid = (u32)std::min<u64>(n_tiles, LQ_GATHER_MAX_BLOCKS);
	if (kind == 1) LQ_LAUNCH(k_bam_gather, grid, LQ_GATHER_THREADS, c.stream, raw, c.gseg.as<GatherSeg>(), c.gtile.as<u32>(), n_tiles, total, dst);
	else if (kind == 2) LQ_LAUNCH(k_bam_qual, grid, LQ_GATHER_THREADS, c.stream, raw, c.gseg.as<GatherSeg>(), c.gtile.as<u32>(), n_tiles, total, dst);
	else LQ_LAUNCH(k_chunk_gather, grid, LQ_GATHER_THREADS, c.stream, raw, c.gseg.as<GatherSeg>(), c.gtile.as<u32>(), n_tiles, total, dst, upper ? 1 : 0);
	LQ_HIP_CHECK(hipGetLastError());
	LQ_HIP_CHECK(hipStreamSynchronize(c.stream));             // (tile_seg dies here, and the two device lists serve the next launch)
}

// the same launch from segments that lie on the device (segs: room for one more entry): the work list is made there too; kind as above
static void gather_launch_dev(lqchunk &c, const u8 *raw, GatherSeg *segs, u64 n_segs, u8 *dst, bool upper, int kind)
{
	const u64 total = c.total;
	if (!total) return;
	const u64 n_tiles = (total + LQ_GATHER_TILE - 1) / LQ_GATHER_TILE;
	if (n_segs > 0xffffffffULL) throw std::domain_error("more than 2^32-1 lines in one chunk");
	if (!n_segs) throw std::logic_error("bases without segments");
	const GatherSeg end = {0, total};
	LQ_HIP_CHECK(hipMemcpyAsync(segs + n_segs, &end, sizeof(end), hipMemcpyHostToDevice, c.stream));
	c.gtile.ensure((n_tiles + 1) * 4);
	const u32 tgrid = (u32)std::min<u64>((n_tiles + 1 + LQ_FXSCAN_THREADS - 1) / LQ_FXSCAN_THREADS, LQ_FXSCAN_TILESEG_MAX_BLOCKS);
	LQ_LAUNCH(k_fx_tileseg, tgrid, LQ_FXSCAN_THREADS, c.stream, (const GatherSeg*)segs, (u32)n_segs, n_tiles, LQ_GATHER_TILE, c.gtile.as<u32>());
	const u32 grid = (u32)std::min<u64>(n_tiles, LQ_GATHER_MAX_BLOCKS);
	if (kind == 1) LQ_LAUNCH(k_bam_gather, grid, LQ_GATHER_THREADS, c.stream, raw, (const GatherSeg*)segs, (const u32*)c.gtile.as<u32>(), n_tiles, total, dst);
	else if (kind == 2) LQ_LAUNCH(k_bam_qual, grid, LQ_GATHER_THREADS, c.stream, raw, (const GatherSeg*)segs, (const u32*)c.gtile.as<u32>(), n_tiles, total, dst);
	else LQ_LAUNCH(k_chunk_gather, grid, LQ_GATHER_THREADS, c.stream, raw, (const GatherSeg*)segs, (const u32*)c.gtile.as<u32>(), n_tiles, total, dst, upper ? 1 : 0);
	LQ_HIP_CHECK(hipGetLastError());
	LQ_HIP_CHECK(hipStreamSynchronize(c.stream));             // (`end` dies here)
}

static void gather_begin(lqchunk &c, const std::vector<u64> &off)
{
	lq_cabi::select_device(c.device);
	if (!c.stream) LQ_HIP_CHECK(hipStreamCreate(&c.stream));
	const u32 n = (u32)(off.size() - 1);
	c.resident = false; c.packed = false; c.n_chunks = 0; c.iv_valid = false; c.dust_done = false; c.cols_done = false;
	c.n = n; c.first_desc = n; c.off = off; c.total = off[n]; c.h_seq = c.h_qual = nullptr; c.has_qual = true;
	// the buffers of lq_chunk_ready; k_chunk_gather writes whole 16-byte words, zeros behind the last base
	const u64 total = c.total, alloc = (total + LQ_CHUNK_SEQ_TILE - 1) / LQ_CHUNK_SEQ_TILE * LQ_CHUNK_SEQ_TILE + LQ_PACK_PAD;
	const u64 words = (total + 15) / 16 * 16;
	c.seq.ensure((size_t)alloc); c.qual.ensure((size_t)total + LQ_GATHER_SRC_PAD); c.d_off.ensure(((size_t)n + 1) * 8);
	LQ_HIP_CHECK(hipMemsetAsync(c.seq.as<u8>() + words, 0, (size_t)(alloc - words), c.stream));
	LQ_HIP_CHECK(hipMemcpyAsync(c.d_off.p, c.off.data(), ((size_t)n + 1) * 8, hipMemcpyHostToDevice, c.stream));
}

void lq_chunk_gather_dev(lqchunk &c, const std::vector<u64> &off, const u8 *raw, GatherSeg *sseg, u64 n_sseg, GatherSeg *qseg, u64 n_qseg, bool upper, int bam)
{
	gather_begin(c, off);
	gather_launch_dev(c, raw, sseg, n_sseg, c.seq.as<u8>(), upper, bam ? 1 : 0);
	gather_launch_dev(c, raw, qseg, n_qseg, c.qual.as<u8>(), false, bam == 2 ? 2 : 0);
	LQ_HIP_CHECK(hipStreamSynchronize(c.stream));
	c.resident = true;
}

void lq_chunk_gather(lqchunk &c, const std::vector<u64> &off, const u8 *raw, std::vector<GatherSeg> &sseg, std::vector<GatherSeg> &qseg, bool upper, int bam)
{
	gather_begin(c, off);
	gather_launch(c, raw, sseg, c.seq.as<u8>(), upper, bam ? 1 : 0);
	gather_launch(c, raw, qseg, c.qual.as<u8>(), false, bam == 2 ? 2 : 0);
	LQ_HIP_CHECK(hipStreamSynchronize(c.stream));
	c.resident = true;
}

namespace {
thread_local std::string g_chunk_create_error;

template <class F> int chunk_guard(lqchunk *c, F &&f)
{
	if (!c) return LQCOV_E_ARG;
	char buf[512] = {0};
	const int rc = lq_cabi::guarded(buf, sizeof(buf), f);
	if (rc) c->err = buf;
	return rc;
}

void need_loaded(const lqchunk &c) { if (!c.resident) throw std::logic_error("no chunk loaded (lqchunk_load)"); }

// the scan's three host arrays come together or not at all (all null: the results stay on the device)
bool some_null(const void *a, const void *b, const void *d) { return (!a || !b || !d) && (a || b || d); }

// ASCII -> the engine's packed layout, on the device
void chunk_pack(lqchunk &c)
{
	need_loaded(c);
	const u32 n = c.n;
	for (u32 i = 0; i < n; ++i) if (c.off[i + 1] - c.off[i] > 0x7fffffffULL) throw std::domain_error("read longer than 2^31-1 bases (bseq.c:80)");
	c.h_coff.assign((size_t)n + 1, 0);
	for (u32 i = 0; i < n; ++i) c.h_coff[i + 1] = c.h_coff[i] + (c.off[i + 1] - c.off[i] + LQ_CHUNK - 1) / LQ_CHUNK;
	c.n_chunks = c.h_coff[n];
	c.packed = true;
	if (!c.n_chunks) return;
	lq_chunk_ready(c);
	const u64 n_words = c.n_chunks * LQ_CHUNK_WORDS, n_tiles = (c.n_chunks + LQ_PACK_TILE_CHUNKS - 1) / LQ_PACK_TILE_CHUNKS;
	std::vector<u32> tile_read((size_t)n_tiles + 1);          // the work list: the read that holds the first chunk of every tile
	{
		u32 r = 0;
		for (u64 t = 0; t < n_tiles; ++t) {
			while (r + 1 < n && c.h_coff[r + 1] <= t * LQ_PACK_TILE_CHUNKS) ++r;
			tile_read[t] = r;
		}
		tile_read[n_tiles] = n - 1;
	}
	c.coff.ensure(((size_t)n + 1) * 8); c.tile_read.ensure((n_tiles + 1) * 4);
	c.codes.ensure(n_words * 8); c.amb.ensure(n_words * 4); c.flags.ensure(n);
	LQ_HIP_CHECK(hipMemcpyAsync(c.coff.p, c.h_coff.data(), ((size_t)n + 1) * 8, hipMemcpyHostToDevice, c.stream));
	LQ_HIP_CHECK(hipMemcpyAsync(c.tile_read.p, tile_read.data(), (n_tiles + 1) * 4, hipMemcpyHostToDevice, c.stream));
	LQ_HIP_CHECK(hipMemsetAsync(c.flags.p, 0, n, c.stream));
	const u32 grid = (u32)std::min<u64>(n_tiles, LQ_PACK_MAX_BLOCKS);
	LQ_LAUNCH(k_chunk_pack, grid, LQ_PACK_THREADS, c.stream, c.seq.as<u8>(), c.d_off.as<u64>(), c.coff.as<u64>(), c.tile_read.as<u32>(), n_tiles, n_words,
	          c.codes.as<u64>(), c.amb.as<u32>(), c.flags.as<u8>());
	LQ_HIP_CHECK(hipGetLastError());
	LQ_HIP_CHECK(hipStreamSynchronize(c.stream));             // (tile_read dies here)
}
} // namespace

// ---- the store -------------------------------------------------------------------------------------------------------------
struct lqstore {
	struct Block {                                            // one appended chunk
		u64 *codes = nullptr; u32 *amb = nullptr;             // device, n_chunks * 32 / 16 bytes; amb == nullptr: no read holds an ambiguous base
		u64 n_chunks = 0;
		std::vector<u32> lens;
		std::vector<u64> coff, name_off;                      // packed chunks / name bytes before read i
		std::vector<u8> flags;
		std::vector<char> names;
		~Block() { if (codes) (void)hipFree(codes); if (amb) (void)hipFree(amb); }
	};
	int device = 0;
	std::vector<std::unique_ptr<Block>> blocks;
	u64 bytes = 0;
};

extern "C" {

lqchunk *lqchunk_create(int device)
{
	try {
		lq_cabi::select_device(device);
		std::unique_ptr<lqchunk> c(new lqchunk());
		c->device = device;
		LQ_HIP_CHECK(hipStreamCreate(&c->stream));
		return c.release();
	} catch (const std::exception &e) { g_chunk_create_error = e.what(); return nullptr; }
}

void lqchunk_destroy(lqchunk *c) { delete c; }

const char *lqchunk_last_error(const lqchunk *c) { return c ? c->err.c_str() : g_chunk_create_error.c_str(); }

int lqchunk_load(lqchunk *c, uint32_t n, const uint8_t *seq, const uint64_t *seq_off, const uint8_t *qual)
{
	return chunk_guard(c, [&] {
		if (!seq_off || (n && seq_off[n] != seq_off[0] && !seq)) throw std::invalid_argument("null buffers");
		c->resident = false;
		for (u32 i = 0; i < n; ++i) if (seq_off[i + 1] < seq_off[i]) throw std::invalid_argument("seq_off is not ascending");
		lq_chunk_set(*c, n, seq, seq_off, qual);
		lq_chunk_ready(*c);
	});
}

int lqchunk_sdust(lqchunk *c, int W, int T, uint32_t *masked, double *qual_psum, uint32_t *n_above_q7)
{
	return chunk_guard(c, [&] {
		need_loaded(*c);
		if (c->n && some_null(masked, qual_psum, n_above_q7)) throw std::invalid_argument("null buffers");
		lq_chunk_sdust(*c, W, T, masked, qual_psum, n_above_q7);
	});
}

int lqchunk_sdust_split(lqchunk *c, int W, int T, uint32_t piece, uint32_t *masked, double *qual_psum, uint32_t *n_above_q7, uint32_t *n_serial)
{
	return chunk_guard(c, [&] {
		need_loaded(*c);
		if (c->n && some_null(masked, qual_psum, n_above_q7)) throw std::invalid_argument("null buffers");
		lq_chunk_sdust_split(*c, W, T, piece, masked, qual_psum, n_above_q7, n_serial);
	});
}

int lqchunk_sdust_table(lqchunk *c, const char *names, const uint64_t *name_off, uint8_t *out, uint64_t out_cap, uint64_t *out_len, lqsdust_stats *stats,
                        uint32_t *excl, uint64_t excl_cap)
{
	return chunk_guard(c, [&] {
		need_loaded(*c);
		if (!out_len) throw std::invalid_argument("null buffers");
		u64 st[LQSDUST_STATS_WORDS] = {0};
		try { lq_chunk_sdust_table(*c, names, name_off, out, out_cap, out_len, st, excl, excl_cap); }
		catch (...) { if (stats) memcpy(stats, st, sizeof(st)); throw; }      // (a table that does not fit: its size and summary are known)
		if (stats) memcpy(stats, st, sizeof(st));
	});
}

int lqchunk_sdust_columns(lqchunk *c, uint32_t *frac_thou, int32_t *qv_thou)
{
	return chunk_guard(c, [&] { need_loaded(*c); lq_chunk_sdust_columns(*c, frac_thou, (i32*)qv_thou); });
}

int lqchunk_sdust_intervals(lqchunk *c, int W, int T, uint32_t piece, uint64_t *n_off, uint8_t *flagged, uint64_t *iv, size_t iv_cap, size_t *iv_need)
{
	return chunk_guard(c, [&] {
		need_loaded(*c);
		if (!n_off || !iv_need) throw std::invalid_argument("null buffers");
		lq_chunk_sdust_intervals(*c, W, T, piece);
		const size_t need = c->h_iv.size();
		*iv_need = need;
		for (u32 i = 0; i <= c->n; ++i) n_off[i] = c->h_ivoff[i];
		if (flagged && c->n) memcpy(flagged, c->h_dflag.data(), c->n);
		if (!iv) return;                                          // (the first of the two calls: the size)
		if (iv_cap < need) throw std::invalid_argument("iv_cap is smaller than the number of intervals (iv_need)");
		if (need) memcpy(iv, c->h_iv.data(), need * 8);
	});
}

int lqchunk_adapt(lqchunk *c, const uint8_t *adp5, uint32_t len5, const uint8_t *adp3, uint32_t len3, uint32_t length, int32_t *out5, int32_t *out3)
{
	return chunk_guard(c, [&] { need_loaded(*c); lq_chunk_adapt(*c, adp5, len5, adp3, len3, length, out5, out3); });
}

int lqchunk_gc(lqchunk *c, uint32_t chunk_size, const uint32_t *k, const uint64_t *draw_off, const uint32_t *pos_in, uint64_t seed, uint64_t first_read,
               uint32_t *gc, uint32_t *pos_out, uint16_t *win_gc, uint32_t *kept)
{
	return chunk_guard(c, [&] { need_loaded(*c); lq_chunk_gc(*c, chunk_size, k, draw_off, pos_in, seed, first_read, gc, pos_out, win_gc, kept); });
}

int lqchunk_pack(lqchunk *c) { return chunk_guard(c, [&] { chunk_pack(*c); }); }

int lqchunk_get_packed(lqchunk *c, uint64_t *codes, uint32_t *amb, uint8_t *amb_flags)
{
	return chunk_guard(c, [&] {
		if (!c->packed) throw std::logic_error("the chunk is not packed (lqchunk_pack)");
		if ((c->n_chunks && (!codes || !amb)) || (c->n && !amb_flags)) throw std::invalid_argument("null buffers");
		if (c->n) memset(amb_flags, 0, c->n);
		if (!c->n_chunks) return;
		lq_cabi::select_device(c->device);
		const u64 n_words = c->n_chunks * LQ_CHUNK_WORDS;
		LQ_HIP_CHECK(hipMemcpyAsync(codes, c->codes.p, n_words * 8, hipMemcpyDeviceToHost, c->stream));
		LQ_HIP_CHECK(hipMemcpyAsync(amb, c->amb.p, n_words * 4, hipMemcpyDeviceToHost, c->stream));
		LQ_HIP_CHECK(hipMemcpyAsync(amb_flags, c->flags.p, c->n, hipMemcpyDeviceToHost, c->stream));
		LQ_HIP_CHECK(hipStreamSynchronize(c->stream));
	});
}

int lqchunk_get_reads(lqchunk *c, uint32_t n_idx, const uint32_t *idx, uint8_t *seq_out, uint8_t *qual_out)
{
	return chunk_guard(c, [&] {
		need_loaded(*c);
		if (qual_out && !c->has_qual) throw std::invalid_argument("the chunk holds no qualities");
		const u32 n = idx ? n_idx : c->n;
		for (u32 i = 0; idx && i < n; ++i) if (idx[i] >= c->n) throw std::invalid_argument("a read index outside the chunk");
		lq_cabi::select_device(c->device);
		u64 at = 0;
		for (u32 i = 0; i < n;) {                                 // runs of consecutive reads travel in one copy
			const u32 r0 = idx ? idx[i] : 0;
			u32 j = idx ? i + 1 : n;
			while (idx && j < n && idx[j] == idx[j - 1] + 1) ++j;
			const u64 a = c->off[r0], b = c->off[r0 + (j - i)];
			if (b > a) {
				if (!seq_out) throw std::invalid_argument("null buffers");
				LQ_HIP_CHECK(hipMemcpyAsync(seq_out + at, c->seq.as<u8>() + a, (size_t)(b - a), hipMemcpyDeviceToHost, c->stream));
				if (qual_out) LQ_HIP_CHECK(hipMemcpyAsync(qual_out + at, c->qual.as<u8>() + a, (size_t)(b - a), hipMemcpyDeviceToHost, c->stream));
			}
			at += b - a; i = j;
		}
		LQ_HIP_CHECK(hipStreamSynchronize(c->stream));
	});
}

lqstore *lqstore_create(int device)
{
	try {
		lq_cabi::select_device(device);
		lqstore *s = new lqstore();
		s->device = device;
		return s;
	} catch (const std::exception &e) { g_chunk_create_error = e.what(); return nullptr; }
}

void lqstore_destroy(lqstore *s)
{
	if (!s) return;
	(void)hipSetDevice(s->device);
	delete s;
}

uint64_t lqstore_bytes(const lqstore *s) { return s ? s->bytes : 0; }

int lqstore_append(lqstore *s, lqchunk *c, const char *names, const uint64_t *name_off)
{
	if (!s) return LQCOV_E_ARG;
	return chunk_guard(c, [&] {
		if (!c->packed) throw std::logic_error("the chunk is not packed (lqchunk_pack)");
		if (c->device != s->device) throw std::invalid_argument("the chunk lives on another device than the store");
		if (c->n && names && !name_off) throw std::invalid_argument("null buffers");
		if (!c->n) return;
		lq_cabi::select_device(s->device);
		std::unique_ptr<lqstore::Block> b(new lqstore::Block());
		const u32 n = c->n;
		b->n_chunks = c->n_chunks;
		b->lens.resize(n); b->flags.assign(n, 0); b->coff = c->h_coff; b->name_off.assign((size_t)n + 1, 0);
		for (u32 i = 0; i < n; ++i) b->lens[i] = (u32)(c->off[i + 1] - c->off[i]);
		for (u32 i = 0; i < n; ++i) {                         // names as NUL-terminated strings, rebased to the block
			const char *nm = names ? names + name_off[i] : "";
			const size_t l = strlen(nm) + 1;
			b->names.insert(b->names.end(), nm, nm + l);
			b->name_off[i + 1] = b->name_off[i] + l;
		}
		bool any_amb = false;
		if (c->n_chunks) {
			LQ_HIP_CHECK(hipMemcpyAsync(b->flags.data(), c->flags.p, n, hipMemcpyDeviceToHost, c->stream));
			LQ_HIP_CHECK(hipStreamSynchronize(c->stream));
			any_amb = std::find(b->flags.begin(), b->flags.end(), (u8)1) != b->flags.end();
		}
		// one allocation of the exact size per array: 0.25 B per base, 0.375 with the bits (a failure leaves the store as it was: b frees what it got)
		const u64 n_alloc = std::max<u64>(c->n_chunks, 1);
		LQ_HIP_CHECK(hipMalloc((void**)&b->codes, n_alloc * 32));
		if (any_amb) LQ_HIP_CHECK(hipMalloc((void**)&b->amb, n_alloc * 16));
		if (c->n_chunks) {
			LQ_HIP_CHECK(hipMemcpyAsync(b->codes, c->codes.p, c->n_chunks * 32, hipMemcpyDeviceToDevice, c->stream));
			if (any_amb) LQ_HIP_CHECK(hipMemcpyAsync(b->amb, c->amb.p, c->n_chunks * 16, hipMemcpyDeviceToDevice, c->stream));
			LQ_HIP_CHECK(hipStreamSynchronize(c->stream));
		}
		s->blocks.emplace_back(std::move(b));
		s->bytes += n_alloc * (any_amb ? 48 : 32);
	});
}

int lqstore_run(lqstore *s, lqcov_handle *h)
{
	if (!s || !h) return LQCOV_E_ARG;
	// the stored reads as one sequence of lengths, cut into index parts by the reference's rule
	std::vector<std::pair<u32, u32>> where;                   // (block, read in block) of every stored read
	for (u32 b = 0; b < s->blocks.size(); ++b) for (u32 i = 0; i < s->blocks[b]->lens.size(); ++i) where.emplace_back(b, i);
	const auto ranges = lq_part_ranges(where.size(), [&](size_t i) { return (u64)s->blocks[where[i].first]->lens[where[i].second]; },
	                                   h->P.batch_size, (u64)h->P.idx_mini_batch);
	for (const auto &rg : ranges) {
		const int part = lqcov_part_begin(h);
		if (part < 0) return part;
		int rc = 0;
		for (size_t i = rg.first; i < rg.second && !rc;) {    // the piece of every stored chunk that lies in the part
			const lqstore::Block &b = *s->blocks[where[i].first];
			const u32 a = where[i].second, e = (u32)std::min<size_t>(b.lens.size(), a + (rg.second - i));
			const u64 chunks = b.coff[e] - b.coff[a];
			const bool amb = b.amb && std::find(b.flags.begin() + a, b.flags.begin() + e, (u8)1) != b.flags.begin() + e;
			rc = lqcov_part_add_packed_shares_dev(h, part, b.codes + b.coff[a] * LQ_CHUNK_WORDS,
			                                      amb ? b.amb + b.coff[a] * LQ_CHUNK_WORDS : nullptr, chunks, 1, &chunks, e - a, b.lens.data() + a,
			                                      b.names.data(), b.name_off.data() + a);
			i += e - a;
		}
		if (!rc) rc = lqcov_part_build(h, part);
		if (!rc) rc = lqcov_part_map(h, part);
		const int rr = lqcov_part_release(h, part);
		if (rc || rr) return rc ? rc : rr;
	}
	return 0;
}

} // extern "C"
