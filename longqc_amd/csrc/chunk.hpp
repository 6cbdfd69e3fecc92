// longqc_amd/csrc/chunk.hpp -- a chunk of reads resident on the device (lqchunk of include/lqcov.h): the bases, the offsets and, if
// given, the qualities go up once; the low-complexity scan (dust.cpp), the adapter search (adapt.cpp), the GC counts (gc.cpp), the
// packing for the coverage engine (chunk.cpp) and the FASTQ writer (writer.cpp) run on those buffers.  The buffer-level entry points lqsdust_reads,
// lqadapt_reads and lqgc_reads are the same steps on a chunk that lives for one call.
#pragma once
#include "lq_cabi.hpp"
#include <string>
#include <vector>

#define LQ_CHUNK_SEQ_TILE 4096u      // the sequence buffer is allocated in whole tiles of k_gc_reads (LQ_GC_TILE)

// what the file reader (reader.cpp) hands to k_chunk_gather (kernels_gather.hpp): a run of the file's raw bytes on the device that
// lands at one place of the chunk's sequence or quality buffer
struct alignas(16) GatherSeg { u64 src, dst; };        // source byte, destination byte of the segment's first byte
#define LQ_GATHER_FILL LQ_U64MAX     // src of a segment without source bytes: '!' (a record without a quality string)
#define LQ_GATHER_SRC_PAD 32u        // bytes the raw buffer extends past its last byte

// the low-complexity table as text (kernels_dust_table.hpp, dust.cpp): the names, the per-row tables, the lists and the text on the device
struct LqDustTab {
	DBuf names, noff, nlen, fthou, qthou, meta, rbytes, rec, unv, patch, ex1, ex2, st, text, cfrac, cqv;
	Prim prim;                                                // the scan of the rows' byte counts
};

struct lqchunk {
	int device = 0;
	hipStream_t stream = nullptr;
	std::string err;
	// the reads: read i = bases off[i] .. off[i + 1] of the buffer (offsets relative to the first base)
	u32 n = 0, first_desc = 0;                                // first_desc: the first i with seq_off[i + 1] < seq_off[i], n if none
	u64 total = 0;
	std::vector<u64> off;
	bool resident = false;                                    // the reads lq_chunk_set described are on the device
	const u8 *h_seq = nullptr, *h_qual = nullptr;             // the caller's bases / qualities (at the first base), until lq_chunk_ready has uploaded them
	bool has_qual = false;
	DBuf seq, qual, d_off;
	DBuf pi, masked, psum, qv, q2p; bool tab_ready = false;   // sdust: scratch, results, meanQ's table
	// sdust in pieces (kernels_dust_split.hpp): the flags, the mask, the work list, and the flagged reads set one behind the other for k_sdust
	DBuf dflag, dmask, ditem, slist, soff, sseq, smasked, spsum, sqv;
	hipStream_t stream2 = nullptr;                            // k_sdust_qual runs here, beside the pieces
	std::vector<u8> h_dflag;                                  // the flags of the mask on the device
	std::vector<u64> h_iv, h_ivoff;                           // lqchunk_sdust_intervals: the runs of that mask, per read
	bool iv_valid = false; int iv_W = 0, iv_T = 0; u32 iv_piece = 0;   // h_iv, h_ivoff and h_dflag are lqchunk_sdust_intervals' for these arguments and the reads loaded now
	DBuf woff, adp5, adp3, out;                               // adapter search: window offsets, adapters, result rows
	DBuf draw_off, gc, pos, win, kept;                        // GC counts
	DBuf coff, tile_read, codes, amb, flags;                  // packed form
	DBuf gseg, gtile;                                         // k_chunk_gather's segments and work list
	DBuf fq_names, fq_noff, fq_be, fq_rec, fq_tile, fq_text;  // k_fastq_format's names and tables (writer.cpp), lqchunk_fastq's text
	LqDustTab tb;                                             // lqchunk_sdust_table
	bool dust_done = false;                                   // masked, psum and qv are a scan's of the reads loaded now
	bool cols_done = false;                                   // tb.fthou, tb.qthou and tb.meta are the table's of that scan (lqchunk_sdust_columns)
	std::vector<u64> h_coff;                                  // packed chunks before read i
	u64 n_chunks = 0; bool packed = false;
	~lqchunk()
	{
		if (stream2) { hipStreamSynchronize(stream2); hipStreamDestroy(stream2); }
		if (stream) { hipStreamSynchronize(stream); hipStreamDestroy(stream); }
	}
};

// describe the reads (nothing goes to the device and nothing is checked but the order of the offsets: each step keeps its own checks,
// in its own order, and uploads when it first needs the device)
void lq_chunk_set(lqchunk &c, u32 n, const u8 *seq, const u64 *seq_off, const u8 *qual);
// select the device, make the stream, upload what lq_chunk_set described (once)
void lq_chunk_ready(lqchunk &c);
// a chunk made on the device from the raw bytes of a file (reader.cpp): read i = bases off[i] .. off[i + 1]; sseg / qseg: the segments
// of the sequence and of the quality buffer, in destination order and without gaps (one entry is appended to each).  Leaves the chunk
// as lq_chunk_set + lq_chunk_ready leave one that has qualities.  bam: 0 the raw bytes are a FASTA/FASTQ file's; 1 a BAM file's, sseg
// names every read's packed sequence (kernels_bam.hpp) and qseg is LQ_GATHER_FILL throughout; 2 qseg names the reads' quality bytes.
void lq_chunk_gather(lqchunk &c, const std::vector<u64> &off, const u8 *raw, std::vector<GatherSeg> &sseg, std::vector<GatherSeg> &qseg, bool upper, int bam = 0);
// the same from segment lists that lie on the device already (the reader's device parse, kernels_fxscan.hpp): n_sseg / n_qseg entries
// in destination order, room for one more behind each; the per-tile work list is made on the device (k_fx_tileseg).  bam: as
// lq_chunk_gather's (the reader's device walk of a BAM file, kernels_bamscan.hpp)
void lq_chunk_gather_dev(lqchunk &c, const std::vector<u64> &off, const u8 *raw, GatherSeg *sseg, u64 n_sseg, GatherSeg *qseg, u64 n_qseg, bool upper, int bam = 0);
// masked, psum, qv: the host's arrays, or all three null -- the results stay on the device (c.masked, c.psum, c.qv) for lq_chunk_sdust_table
void lq_chunk_sdust(lqchunk &c, int W, int T, u32 *masked, double *psum, u32 *qv);
// the same table with the reads of A/C/G/T alone cut into pieces of `piece` bases (0: LQ_DUST_SPLIT_PIECE), the others walked by k_sdust;
// n_serial (may be null): how many those were
void lq_chunk_sdust_split(lqchunk &c, int W, int T, u32 piece, u32 *masked, double *psum, u32 *qv, u32 *n_serial);
// the maximal runs of the pieces' mask per read (start << 32 | finish; none for a flagged read), kept in c.h_iv / c.h_ivoff / c.h_dflag
void lq_chunk_sdust_intervals(lqchunk &c, int W, int T, u32 piece);
// the table of the last scan as text (dust.cpp); stats: LQSDUST_STATS_WORDS words; excl (may be null): the reads on LongQC's exclusion lists
void lq_chunk_sdust_table(lqchunk &c, const char *names, const u64 *name_off, u8 *out, u64 out_cap, u64 *out_len, u64 *stats, u32 *excl, u64 excl_cap);
// the two "%.3f" columns of that table as thousandths (n entries each; "-nan": 0xffffffff / INT32_MIN)
void lq_chunk_sdust_columns(lqchunk &c, u32 *frac_thou, i32 *qv_thou);
void lq_chunk_adapt(lqchunk &c, const u8 *adp5, u32 len5, const u8 *adp3, u32 len3, u32 length, i32 *out5, i32 *out3);
void lq_chunk_gc(lqchunk &c, u32 chunk_size, const u32 *k, const u64 *draw_off, const u32 *pos_in, u64 seed, u64 first_read,
                 u32 *gc, u32 *pos_out, u16 *win_gc, u32 *kept);
