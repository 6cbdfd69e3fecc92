/* include/lqcov.h -- C ABI of liblqcov.so: the MI355X-native stand-in for LongQC's
 * `minimap2-coverage` subprocess (the hot path behind `longQC.py sampleqc`).
 *
 * The reference has no FFI for this path: the boundary is a process boundary --
 * lq_exec.py:13-38 (`LqExec.exec(*argv, out=, err=)` -> Popen) driven by longQC.py:438-446 and
 * polled at longQC.py:520-526; the C side of it is `main` (minimap2-coverage.c:206) and, one level
 * down, the in-process seam `lq_map_file` (minimap2-coverage.h:41-42; lqmap.c:852).  This header
 * therefore offers two levels, each citing what it replaces:
 *
 *   1. lqcov_main / lqcov_run_files     == the subprocess: same argv in, same 9-column table out
 *                                          (minimap2-coverage.c:166-195 options, :545-617 rows).
 *   2. handle + read-set + part calls    == main's body (minimap2-coverage.c:406-458) and
 *                                          lq_map_file (lqmap.c:852): caller owns the reads, the
 *                                          library owns the device state and the accumulators.
 *
 * All pointers are plain host pointers unless a name ends in _dev (HIP device pointers, used by
 * bench.py and the multi-GPU driver to keep data resident / exchange it over RCCL).  No torch or
 * C++ types cross this boundary.  Every int-returning call yields 0 on success and a negative
 * LQCOV_E_* code on failure; the message is available from lqcov_last_error().  Handles are not
 * thread-safe; one handle drives one HIP device and one stream.
 */
#ifndef LQCOV_H
#define LQCOV_H
#include <stdint.h>
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif

#define LQCOV_ABI_VERSION 1

#define LQCOV_E_ARG     (-1)   /* bad argument / bad option value                     */
#define LQCOV_E_IO      (-2)   /* cannot open / read / write a file                   */
#define LQCOV_E_DEVICE  (-3)   /* HIP error (no device, out of memory, launch failed) */
#define LQCOV_E_STATE   (-4)   /* call sequence violated                              */
#define LQCOV_E_DOMAIN  (-5)   /* input outside the supported domain  */
#define LQCOV_EOF       (-100) /* lqcov_part_load: no further part in the file        */

typedef struct lqcov_handle lqcov_handle;

/* Effective parameters == what minimap2-coverage echoes on stderr (minimap2-coverage.c:392-404).
 * Defaults are the binary's own (minimap2-coverage.c:252-388, map.c:12-44, index.c:31-37). */
typedef struct lqcov_params {
	int32_t  k;                /* -k  (default 12)                                   */
	int32_t  w;                /* -w  (default 5)                                    */
	int32_t  hpc;              /* -H  homopolymer-compressed k-mers                  */
	uint64_t batch_size;       /* -I  bases per index part (default 4G)              */
	int32_t  idx_mini_batch;   /* 50,000,000: part boundaries fall on these (index.c:35,244) */
	int32_t  max_gap;          /* -g  (default 10000), both axes                     */
	int32_t  min_cnt;          /* -n  (default 3)                                    */
	int32_t  min_chain_score;  /* -m  (default 40)                                   */
	int32_t  min_score_med;    /* -p  (default m)                                    */
	int32_t  min_score_good;   /* -q  (default m)                                    */
	int32_t  max_chain_skip;   /* -s  (default 25)                                   */
	int32_t  bw;               /* 500 (map.c:20)                                     */
	int32_t  max_overhang;     /* -a  (default 2000)                                 */
	int32_t  min_ovlp;         /* -l  (default 1000; parsed, unused by lq_cnt_match) */
	int32_t  min_coverage;     /* -c  (default 3)                                    */
	double   min_ratio;        /* -r  (default 0.4)                                  */
	float    mid_occ_frac;     /* 2e-4f (map.c:16)                                   */
	int32_t  no_self;          /* -Y or -X: skip the self diagonal (lqmap.c:185)     */
	int32_t  ava;              /* -X: also skip cmp>0 pairs (lqmap.c:187)            */
	int32_t  filter_flag;      /* --filter row format (minimap2-coverage.c:586-588)  */
	int32_t  n_threads;        /* -t: accepted, ignored (the device is the pool)     */
} lqcov_params;

/* One output row before text formatting (minimap2-coverage.c:545-605). Regions live in the pools
 * returned by lqcov_get_regions(). */
typedef struct lqcov_row {
	uint64_t lambda;           /* column 3  */
	uint64_t lambda2;          /* numerator of column 9 */
	double   qual_psum;        /* sum of q2p[q-33] over the read (lqutils.c:51-56); NaN-free, host takes log10 */
	uint32_t qlen;             /* column 2  */
	uint32_t n_mini;           /* mv.n      (minimap2-coverage.c:422) */
	uint32_t n_match;          /* #counters above the integer mean (minimap2-coverage.c:552-561) */
	float    avg_k;            /* esterr.c:93-97 */
	uint32_t reg_off, n_reg;   /* regs  (column 4) */
	uint32_t mreg_off, n_mreg; /* mregs (column 5) */
	uint32_t has_qual;         /* 0 for FASTA queries: meanQ prints as the reference's NaN */
	uint32_t flags;            /* LQCOV_ROW_* */
} lqcov_row;
#define LQCOV_ROW_SATURATED 1u /* a uint16 match counter reached 65535: esterr.c:130,136 make the result depend on the order of the chains */
#define LQCOV_ROW_REPLAYED  4u /* ... and the query's counters were replayed in the reference's chain order (hit.c:52-88): the row is exact.
                                  SATURATED without REPLAYED (counters merged from several ranks): row not guaranteed */

typedef struct lqcov_region { uint32_t start, end; } lqcov_region;

/* Per-stage device time of the calls made so far on the handle (ms, HIP events on the handle's
 * stream); filled when profiling was switched on with lqcov_set_profiling(). */
typedef struct lqcov_stage_time {
	char     name[48];
	double   total_ms;
	uint64_t launches;
	uint64_t algo_bytes;       /* algorithmic (compulsory) bytes moved, SURVEY.md section 8(d) */
} lqcov_stage_time;

/* ---- level 1: the subprocess ------------------------------------------------------------- */
/* == `minimap2-coverage argv...` with stdout -> out_path (NULL: stdout), stderr -> err_path
 * (NULL: stderr).  Returns the process exit status the reference would give (0 / 1), or a
 * negative LQCOV_E_* for device errors.                         minimap2-coverage.c:206-734 */
int lqcov_main(int argc, const char *const *argv, const char *out_path, const char *err_path, int device);

/* same, on an existing handle and with explicit paths (NULL out: stdout, NULL err: stderr) */
int lqcov_run_files(lqcov_handle *h, const char *target_path, const char *query_path, const char *out_path, const char *err_path);
/* same with the reference's -d: every index part is also appended to dump_path in the reference's .mmi layout
 * (mm_idx_dump, index.c:390-426); query_path may be NULL (index only, minimap2-coverage.c:460-468).  target_path may
 * itself be such a file -- from the reference or from here -- (mm_idx_load, index.c:428-479): its k, w and -H then
 * override the handle's for the mapping, as in the reference (index.c:529-531).                                        */
int lqcov_run_files_ex(lqcov_handle *h, const char *target_path, const char *query_path, const char *dump_path,
                       const char *out_path, const char *err_path);

/* lqcov_run_files for n_sets query files at once, set s mapped with -p med[s] / -q good[s] and its table written to out_paths[s]:
 * the targets (plain, gzip or a prebuilt .mmi) are read, sketched and indexed once for all sets.  Each file is parsed as
 * lqcov_run_files parses one; sets with qualities and sets without cannot be mixed (LQCOV_E_DOMAIN).  err_path gets the
 * parameter echo and one line per set with its -p / -q.  No index dump. */
int lqcov_run_files_sets(lqcov_handle *h, const char *target_path, uint32_t n_sets, const char *const *query_paths,
                         const int32_t *med, const int32_t *good, const char *const *out_paths, const char *err_path);

/* ---- level 2: handle ---------------------------------------------------------------------- */
void lqcov_params_default(lqcov_params *p);                                /* minimap2-coverage.c:229-388 */
/* parse the reference's option table; fills target/query with pointers into argv.   :166-197 */
int  lqcov_parse_args(int argc, const char *const *argv, lqcov_params *p, const char **target, const char **query,
                      const char **dump_path, char *errbuf, size_t errbuf_len);
lqcov_handle *lqcov_create(const lqcov_params *p, int device);            /* NULL if no HIP device */
void lqcov_destroy(lqcov_handle *h);
const char *lqcov_last_error(const lqcov_handle *h);
int  lqcov_abi_version(void);
int  lqcov_set_profiling(lqcov_handle *h, int on);                         /* 0 off; 1 wait for every kernel (exclusive per-kernel times); 2 record events only, no waits */
int  lqcov_set_profiling_only(lqcov_handle *h, const char *stage);         /* time only the named stage (NULL / "": all) */
int  lqcov_set_debug(lqcov_handle *h, unsigned flags);                     /* bit0: record chains for lqcov_get_chains; bit1: record every anchor sort for lqcov_get_sort_batches */
int  lqcov_get_stage_times(lqcov_handle *h, lqcov_stage_time *out, int max_out);   /* returns count */

/* Query reads (the subsample): n reads, bases seq[seq_off[i] .. seq_off[i+1]) as ASCII, optional
 * qualities with the same offsets, names as n NUL-terminated strings name[name_off[i]...].
 * Uploads, 2-bit packs and sketches them; sizes the per-query accumulators.
 * == main pass 1 (minimap2-coverage.c:406-444) + mm_bseq_read2 (bseq.c:68-102).              */
int lqcov_set_queries(lqcov_handle *h, uint32_t n, const uint8_t *seq, const uint64_t *seq_off,
                      const uint8_t *qual, const char *names, const uint64_t *name_off);

/* Several query sets mapped in one pass over the targets, each with its own -p / -q (LongQC's `sampleqc --short` runs two calls
 * that differ only in the query file and -p, longQC.py:438-445,527-543; its spike-in filter runs one per subsample,
 * longQC.py:553-575).  The reads are those of lqcov_set_queries for the concatenation of the sets in set order: set s holds the
 * queries set_first[s] .. set_first[s + 1] - 1 (set_first[0] == 0, set_first[n_sets] == n; a set may be empty) and is mapped with
 * -p min_score_med[s], -q min_score_good[s], checked as the option parser checks one call (>= -m, -q >= -p, < 65536).  The
 * 500-Mbase query mini-batch rule applies to each set.  Every other option is the handle's.  Each query is mapped on its own
 * against a part, so every set's rows are those of a call of its own.  lqcov_set_queries is the case of one set. */
int lqcov_set_query_sets(lqcov_handle *h, uint32_t n, const uint8_t *seq, const uint64_t *seq_off, const uint8_t *qual,
                         const char *names, const uint64_t *name_off, uint32_t n_sets, const uint32_t *set_first /* n_sets + 1 */,
                         const int32_t *min_score_med, const int32_t *min_score_good);
int lqcov_n_query_sets(const lqcov_handle *h);       /* 1 after lqcov_set_queries */

/* Index parts == iterations of the loop at minimap2-coverage.c:449-458.  The caller decides the
 * part boundaries (lqcov_run_files applies the reference's rule, index.c:244,311-316). */
int lqcov_part_begin(lqcov_handle *h);                                     /* returns part id >= 0 */
int lqcov_part_add_targets(lqcov_handle *h, int part, uint32_t n, const uint8_t *seq, const uint64_t *seq_off,
                           const char *names, const uint64_t *name_off);   /* == mm_idx_gen step 0 (index.c:240-288) */
/* The same reads handed over 2-bit packed, as the parser thread of lqcov_run_files does it (0.375 B per base cross
 * PCIe instead of the ASCII byte; seq_nt4_table, sketch.c:8-25).  Layout: every read starts on a 128-base chunk; a chunk
 * is 4 x uint64 of codes (base j of a word at bits 2j..2j+1) in `codes` and 4 x uint32 of "not A/C/G/T/U" bits in `amb`
 * (bits beyond the read's end set).  lqcov_packed_chunks gives the chunk count of n reads, lqcov_pack_reads fills
 * caller-owned buffers of 32 / 16 bytes per chunk on the host (n_threads <= 0: up to 16), lqcov_host_alloc / _free hand
 * out page-locked host memory so that the upload runs at PCIe speed.                                               */
uint64_t lqcov_packed_chunks(uint32_t n, const uint64_t *seq_off);
int   lqcov_pack_reads(uint32_t n, const uint8_t *seq, const uint64_t *seq_off, uint64_t *codes, uint32_t *amb, int n_threads);
void *lqcov_host_alloc(size_t bytes);
void  lqcov_host_free(void *p);
int lqcov_part_add_packed(lqcov_handle *h, int part, uint32_t n, const uint64_t *codes, const uint32_t *amb, const uint32_t *lens,
                          const char *names, const uint64_t *name_off);
/* amb == NULL in lqcov_part_add_packed: none of the n reads holds an ambiguous base -- only `codes` crosses PCIe (0.25 B per base) and the
 * device makes the bits beyond the reads' ends itself.  lqcov_packed_ambiguous_reads says which reads of a packed set do hold one
 * (flags[i] = 1: a bit of `amb` below read i's length is set), so that a caller can tell for any range of reads.  (seq_nt4_table,
 * sketch.c:8-25: an ambiguous base resets mm_sketch's k-mer, sketch.c:114.) */
int lqcov_packed_ambiguous_reads(uint32_t n, const uint32_t *amb, const uint32_t *lens, uint8_t *flags);
/* The same reads from DEVICE memory, in shares: share i (share_chunks[i] 128-base chunks, a whole number of reads) starts at chunk
 * i * stride_chunks of codes_dev (4 x u64 per chunk) / amb_dev (4 x u32 per chunk); the shares are copied back to back in
 * share order = read order.  For a host that received the packed reads of a part from its peers (the query-sharded multi-GPU
 * split all-gathers 0.375 B per base over RCCL instead of 16 B per minimizer): lens / names describe every read of the part.
 * amb_dev == NULL: as amb == NULL above.  A part may be filled by several calls, each appending its reads behind those already there
 * and each with an amb_dev or without (lqstore_run: the pieces of the stored chunks a part is made of).  No counterpart in the
 * reference (its parts come from one file, bseq.c:68-102). */
int lqcov_part_add_packed_shares_dev(lqcov_handle *h, int part, const uint64_t *codes_dev, const uint32_t *amb_dev, uint64_t stride_chunks,
                                     uint32_t n_shares, const uint64_t *share_chunks, uint32_t n, const uint32_t *lens,
                                     const char *names, const uint64_t *name_off);
int lqcov_part_clear(lqcov_handle *h, int part);    /* forget the part's reads and index, keep its device buffers (bench: the same part object every step) */
int lqcov_part_build(lqcov_handle *h, int part);    /* sketch + index (+ mid_occ once): index.c:291-330, map.c:46-54 */
int lqcov_part_map(lqcov_handle *h, int part);      /* == lq_map_file (lqmap.c:852): accumulates into the handle */
int lqcov_part_release(lqcov_handle *h, int part);  /* == mm_idx_destroy (minimap2-coverage.c:457) */
/* .mmi parts.  lqcov_part_dump writes a built part in the reference's layout (append != 0: after the parts already in
 * the file).  lqcov_part_load reads the part that starts at *offset of an .mmi file into a new, built part: returns its
 * id and advances *offset; LQCOV_EOF when no part starts there; the file's k / w / -H must be the handle's.            */
int lqcov_part_dump(lqcov_handle *h, int part, const char *path, int append);               /* index.c:390-426 */
int lqcov_part_load(lqcov_handle *h, const char *path, uint64_t *offset);                   /* index.c:428-479 */
int lqcov_reset(lqcov_handle *h);                   /* zero the accumulators, keep resident reads (bench) */
int lqcov_sync(lqcov_handle *h);                    /* wait for the handle's stream */
/* One part can be built while another is mapped: lqcov_part_add_* / lqcov_part_sketch / lqcov_part_build on one part object
 * from one host thread, lqcov_part_map on another part object from another thread (upload, sketch and index run on a stream
 * and scratch of their own).  mm_idx_reader_read + the mapping of the previous part in a pipeline (minimap2-coverage.c:449-458
 * runs them one after the other).  The mapping lanes size their work space from the HBM that is free when the first part is
 * mapped: tell the engine how much to leave for the part that will be built meanwhile. */
int lqcov_reserve_hbm(lqcov_handle *h, uint64_t bytes);

/* Hand the work space the mapping lanes keep between calls (HIP's stream-ordered pool, kept so that the next part does not
 * pay for it again) back to the device: for a host that needs the HBM for buffers of its own between two parts, e.g. the
 * all-gather buffers of the query-sharded multi-GPU split.  Waits for the device.  No counterpart in the reference. */
int lqcov_workspace_trim(lqcov_handle *h);

/* == main pass 2 up to, not including, printf (minimap2-coverage.c:545-566). */
int lqcov_finish(lqcov_handle *h);
int lqcov_n_queries(const lqcov_handle *h);
/* The engine holds the queries longest first; perm[i] = the caller's index of the i-th query in that order.  Only the
 * per-query arrays of lqcov_accum_export_dev / lqcov_accum_import_dev are in the engine's order; rows, regions, minimizer
 * and chain dumps are in the caller's. */
int lqcov_query_order(lqcov_handle *h, uint32_t *perm, uint32_t n);
int lqcov_get_rows(lqcov_handle *h, lqcov_row *rows, uint32_t n_rows);
int lqcov_get_regions(lqcov_handle *h, const lqcov_region **regs, uint32_t *n_regs, const lqcov_region **mregs, uint32_t *n_mregs);
/* Text of the table, rows in query order (minimap2-coverage.c:567-605). names as in lqcov_set_queries. */
int lqcov_write_table(lqcov_handle *h, const char *out_path);
/* The rows of one query set, in that set's order: the table a call of its own would print (for two sets, lqcov_write_table is
 * their concatenation, LongQC's merged_coverage_out.txt, longQC.py:527-543). */
int lqcov_write_table_set(lqcov_handle *h, uint32_t set, const char *out_path);

/* ---- parity / inspection ------------------------------------------------------------------ */
int32_t  lqcov_mid_occ(const lqcov_handle *h);                             /* map.c:50 */
uint64_t lqcov_part_n_minimizers(const lqcov_handle *h, int part);
uint64_t lqcov_part_n_keys(const lqcov_handle *h, int part);
uint64_t lqcov_last_n_anchors(const lqcov_handle *h);
/* What the mapping did with the seed hits (collect_seed_hits, lqmap.c:140-205 / radix_sort_128x, lqmap.c:238), for logs and
 * benchmarks: out[0] = anchors written against the last part (the hits whose (strand, target) can reach a chain), out[1..3] =
 * since lqcov_reset: runs chained in klib's own order of equal-x anchors, the queries that own them, the anchors those
 * queries were sorted by klib's passes for.  No counterpart in the reference (it writes and sorts every hit). */
void lqcov_map_stats(const lqcov_handle *h, uint64_t out[4]);
/* Why runs were left to klib's own order (since lqcov_reset; a run is counted once, by the first reason found -- the rule is in
 * kernels_chain.hpp, TieGroup, and restates where mm_chain_dp, chain.c:41-108, can see the order radix_sort_128x, lqmap.c:238, leaves
 * equal-x anchors in): out[0] a skip was pending when a group of tied candidates began (chain.c:72-74), out[1] a member of the
 * group counts as a skip, out[2] the group's top score is reached by two members (chain.c:69-71: max_j), out[3] the scan broke off
 * (chain.c:73) before a tie partner that would have raised the best score, out[4] two equal-x peaks of one score in the backtrack
 * order (chain.c:102-108), out[5] other.  No counterpart in the reference. */
void lqcov_tie_reasons(const lqcov_handle *h, uint64_t out[6]);
/* The records of a FASTA/FASTQ file as the target reader sees them (kseq_read + the U -> T of kseq2bseq, kseq.h:179-224,
 * bseq.c:56-66): out[0] = records, out[1] = bases, out[2] = a hash over the names, out[3] = a hash over the sequences, out[4] =
 * pieces of the file that had to be parsed again in order (parallel reader only).  mode 0: the streaming reader (one thread,
 * also gzip); mode 1: the reader over the mapped file with n_threads threads and pieces of piece_bytes (plain files only:
 * LQCOV_E_ARG otherwise).  Both must agree on every input -- that is what this call is for (tests); no device needed. */
int lqcov_fastx_digest(const char *path, int mode, int n_threads, uint64_t piece_bytes, uint64_t out[5]);
/* minimizers of the query set / of a part, reference encoding (sketch.c:70-72): xy[2*i], xy[2*i+1];
 * off[n+1] per-read offsets.  Pass NULL buffers to get the total in *n_total. */
int lqcov_get_query_minimizers(lqcov_handle *h, uint64_t *xy, uint64_t *off, uint64_t *n_total);
int lqcov_get_part_minimizers(lqcov_handle *h, int part, uint64_t *xy, uint64_t *off, uint64_t *n_total);
/* chains of the last lqcov_part_map call: 9 int32 per chain
 * (query, rid, rev, score, cnt, qs, qe, rs, re), unordered. */
int lqcov_get_chains(lqcov_handle *h, int32_t *out, uint64_t cap, uint64_t *n_total);
/* The seed plan of a built part (made by lqcov_part_build when the queries are set; read-only, nothing is computed): the seed
 * hits that can be part of a chain at all, as the first pass will write them.  info[0] = 1 if the plan holds filtered
 * survivors (0: no filter ran, the first pass writes every hit, and there are no rows), info[1] = the hits a chain needs at
 * least (n_min), info[2], info[3] = the queries [q_begin, q_end) the plan holds right now, in the engine's own order
 * (lqcov_query_order).  off[0 .. q_end - q_begin] (up to off_cap entries): where every query's rows start.  rows (up to
 * row_cap rows): 5 uint32 per survivor, in the order the plan keeps them -- query (engine order), target, relative strand,
 * diagonal (target position - query coordinate + query length + 256), minimizer index inside the query.  *n_rows: the rows
 * the plan holds; pass NULL buffers to get the sizes. */
int lqcov_part_seed_survivors(lqcov_handle *h, int part, uint32_t info[4], uint64_t *off, uint64_t off_cap, uint32_t *rows, uint64_t row_cap, uint64_t *n_rows);

/* Saturated uint16 match counters with the index parts spread over ranks (esterr.c:127-138: once a counter is at 65535 the
 * others depend on the order in which lq_cnt_match met the chains, hit.c:52-88 -- on one handle the engine replays that by
 * itself).  The ranks see a counter reach the limit only in the merged sums; then, for that query (engine order:
 * lqcov_query_order) and every part of the round in part order:
 *   lqcov_part_sat_records   on the rank that mapped the part: the query is chained once more against it, every kept chain
 *                            recorded (records of lqcov_sat_record_bytes() bytes + a pool of counter indices); call with
 *                            recs == NULL to get the two counts in n_out first (the chaining is done once and kept);
 *   lqcov_sat_replay         on every rank, host arithmetic only: the records replayed in the reference's order on the query's
 *                            counters (lqcov_counter_offsets: counters[off[q]] .. counters[off[q + 1] - 1] of the exported
 *                            array) as they stood before the part; lqcov_counter_max: 65535 (the uint16 limit);
 *   lqcov_accum_set_replayed after lqcov_accum_import_dev: these counters take the place of the merged sums, the row carries
 *                            LQCOV_ROW_REPLAYED. */
uint32_t lqcov_sat_record_bytes(void);
uint32_t lqcov_counter_max(const lqcov_handle *h);
int lqcov_counter_offsets(lqcov_handle *h, uint64_t *off /* n_queries + 1 */);
int lqcov_part_sat_records(lqcov_handle *h, int part, uint32_t query, void *recs, uint64_t rec_cap, uint32_t *at, uint64_t at_cap, uint64_t n_out[2]);
int lqcov_sat_replay(lqcov_handle *h, uint32_t query, const void *recs, uint64_t n_recs, const uint32_t *at, uint64_t n_at,
                     uint32_t *counters, uint64_t n_counters);
int lqcov_accum_set_replayed(lqcov_handle *h, uint32_t query, const uint32_t *counters, uint64_t n_counters);

/* Test access to the engine's device-wide primitives (kernels_isort.hpp; they stand where the reference calls klib's
 * radix_sort_128x on a bucket of minimizers, index.c:150-201): a stable sort of n (key, value) pairs by the low `bits` bits of
 * the keys (key_bytes 4: the keys travel as 32-bit words, as for k <= 16; 8: as 64-bit words; vals == NULL: keys only, 4-byte
 * keys), and out[i] = sum of in[0..i-1].  Host arrays in and out. */
int lqcov_debug_sort_pairs(lqcov_handle *h, uint64_t *keys, uint64_t *vals, uint64_t n, unsigned bits, int key_bytes);
int lqcov_debug_scan(lqcov_handle *h, const uint32_t *in, uint64_t *out, uint64_t n);

/* Test access to the anchor sort between the seed stage and the chains (lqmap.c:238): sort_batch on anchors handed
 * in from the host.  xy: n anchors (x, y) as the seed stage would emit them, query after query (q_off: n_q + 1 offsets from 0
 * to n); on return the sorted anchors.  q_klib[q] = 1: query q goes through klib's passes (more than 64 anchors), 0: it holds no
 * equal x, or at most 64 anchors.  n_targets, max_len: the geometry of the part the anchors are said to come from -- it decides
 * which key bytes the passes step over; every anchor must lie inside it (rid < n_targets, position < max_len), n < 2^31,
 * otherwise LQCOV_E_ARG.  want != NULL: the second pass's pruning, with the sorted keys query << 32 | x >> 32 of the runs that
 * are wanted (queries numbered 0 .. n_q - 1): only those runs are promised to be there, in klib's order, and the keys x >> 32
 * of every query still ascend.  With profiling on, lqcov_get_stage_times names the kernels that ran.  (LQCOV_DEBUG_SORT and
 * lqcov_set_debug's bit 1 switch the pruning off here as they do in a mapping.) */
int lqcov_debug_sort_anchors(lqcov_handle *h, uint64_t *xy, uint64_t n, const uint64_t *q_off, const uint32_t *q_klib, uint32_t n_q,
                             uint32_t n_targets, uint32_t max_len, const uint64_t *want, uint32_t n_want);
/* Test access to the stage between the chains and the persisted intervals (filter_redundant_coords, lqmap.c:25-100, as a part's
 * batch runs it: split, sort by query, offsets, room in the pool, the filter).  intervals: n triples (query in the engine's order,
 * start, end), host array, laid out as lqcov_accum_export_dev hands intervals out and encoded as the chains emit them
 * (position << 3 | flags, esterr.c:122-125), in any order: one part's intervals of these queries.  What the filter keeps, and the
 * markers it makes, are appended to the handle's persisted intervals (lqcov_accum_export_dev shows them, lqcov_finish sweeps
 * them).  The pool is not grown ahead as lqcov_part_map does.  info[0] = the persisted intervals afterwards, info[1] = 1 if this
 * call had to move the earlier ones to a larger pool.  A query >= lqcov_n_queries is LQCOV_E_ARG. */
int lqcov_debug_filter_intervals(lqcov_handle *h, const uint32_t *intervals, uint32_t n, uint32_t info[2]);
/* What the last lqcov_part_map handed to the anchor sort, call by call (lqcov_set_debug bit 1; nothing is kept without it, and
 * while it is set the second pass sorts its queries whole, without pruning).  info[0] = the number of recorded sorts,
 * and for sort `index`: info[1] = its kind (0: every seed hit in klib's order -- LQCOV_TIES=klib, or the replay of a saturated
 * query; 1: first pass, the seed filter's survivors, equal x in any order; 2: second pass), info[2] = its queries n_q.
 * q, klib (up to q_cap entries): the engine's query numbers (lqcov_query_order) and which of them went through klib's passes;
 * off (up to q_cap entries of n_q + 1): where every query's anchors start; emitted, sorted (up to a_cap anchors of two words):
 * the anchors as the seed stage wrote them and as the sort left them.  *n_anchors: the anchors of the sort; pass NULL buffers to
 * get the sizes.  An index past the last sort sets info[0] alone. */
int lqcov_get_sort_batches(lqcov_handle *h, uint32_t index, uint32_t info[4], uint32_t *q, uint32_t *klib, uint64_t *off, uint64_t q_cap,
                           uint64_t *emitted, uint64_t *sorted, uint64_t a_cap, uint64_t *n_anchors);

/* The table text (minimap2-coverage.c:567-605) of rows computed elsewhere: the ranks of a multi-GPU run gather their rows and
 * region pools as they are (lqcov_get_rows / lqcov_get_regions; reg_off / mreg_off rebased onto the concatenated pools) and
 * one rank prints them.  No handle: formatting needs nothing but the rows.  names: n_rows NUL-terminated strings. */
int lqcov_format_rows(int filter_flag, const lqcov_row *rows, uint32_t n_rows, const lqcov_region *regs, const lqcov_region *mregs,
                      const char *names, const uint64_t *name_off, const char *out_path);

/* ---- multi-GPU plumbing (device pointers; torch.distributed/RCCL moves the bytes) ----------- */
/* minimizers of a built part as two device arrays (x = hash<<8|span, y = rid<<32|pos<<1|strand) */
int lqcov_part_minimizers_dev(lqcov_handle *h, int part, const uint64_t **x_dev, const uint64_t **y_dev, uint64_t *n);
/* the same into caller-owned device buffers of `cap` entries each (e.g. the send buffers of an all-gather), with rid_base
 * added to every rid: the part-global index of this rank's first read */
int lqcov_part_minimizers_export_dev(lqcov_handle *h, int part, uint64_t *x_dev, uint64_t *y_dev, uint64_t cap, uint32_t rid_base);
/* sketch only (no index): step 1 of mm_idx_gen (index.c:291-302) on this rank's share of the part */
int lqcov_part_sketch(lqcov_handle *h, int part);
/* replace the part's minimizer set by caller-provided device arrays (rank-concatenated, y-sorted),
 * with the part-global target lengths and names, then (re)build the index from them */
int lqcov_part_build_from_minimizers_dev(lqcov_handle *h, int part, const uint64_t *x_dev, const uint64_t *y_dev, uint64_t n,
                                         uint32_t n_targets, const uint32_t *target_len, const char *names, const uint64_t *name_off);
/* the same from the receive buffers of an all-gather with equally sized send buffers: share i (the minimizers of rank i's reads,
 * share_n[i] <= stride entries, host array) starts at word i * stride of x_dev / y_dev; the shares are copied back to back
 * (read order: mm_idx_gen's order, index.c:291-302) -- no concatenated copy on the caller's side */
int lqcov_part_build_from_minimizer_shares_dev(lqcov_handle *h, int part, const uint64_t *x_dev, const uint64_t *y_dev, uint64_t stride,
                                               uint32_t n_shares, const uint64_t *share_n,
                                               uint32_t n_targets, const uint32_t *target_len, const char *names, const uint64_t *name_off);

/* Index parts on different GPUs == the reference's own -I partitioning (minimap2-coverage.c:449-458) run in
 * parallel.  Parts only interact through (i) mid_occ, frozen from part 0 (map.c:50), (ii) the COVT cap, which
 * drops part p for a query whose lambda/qlen already exceeds 150 (esterr.c:87), and (iii) avg_k, set by the first
 * part that sees the query (esterr.c:93-97).  In distributed mode a handle therefore maps its part with fresh
 * accumulators and no cap; the driver (longqc_amd/multigpu.py) exchanges the per-part accumulators over RCCL,
 * replays (ii) and (iii) in part order, and imports the sums for lqcov_finish().                            */
int lqcov_set_distributed(lqcov_handle *h, int on);
int lqcov_set_mid_occ(lqcov_handle *h, int32_t mid_occ);
int lqcov_accum_sizes(lqcov_handle *h, uint32_t *n_queries, uint64_t *n_counters, uint32_t *n_intervals);
/* copy the accumulators to caller-owned device buffers: lambda/lambda2 [n_queries] u64, avg_k [n_queries] f32,
 * flags [n_queries] u32, counters [n_counters] u32 with their query index counter_owner [n_counters] u32,
 * intervals [n_intervals][3] u32 = (query, start, end) encoded as lqmap.c:69-71.  NULL pointers are skipped. */
int lqcov_accum_export_dev(lqcov_handle *h, uint64_t *lambda_dev, uint64_t *lambda2_dev, float *avg_k_dev, uint32_t *flags_dev,
                           uint32_t *counters_dev, uint32_t *counter_owner_dev, uint32_t *intervals_dev);
int lqcov_accum_import_dev(lqcov_handle *h, const uint64_t *lambda_dev, const uint64_t *lambda2_dev, const float *avg_k_dev, const uint32_t *flags_dev,
                           const uint32_t *counters_dev, const uint32_t *intervals_dev, uint32_t n_intervals);

/* ---- the reference's second binary, `sdust` (low-complexity table of every read) ---------------- */
/* == `sdust [-w W] [-t T] <in.fa|fq[.gz]>` with stdout -> out_path (NULL: stdout), stderr -> err_path: one row per read,
 * name, masked bases, length, masked/length %.3f, meanQ %.3f, #qualities above Q7.            sdust.c:181-222 */
int lqsdust_main(int argc, const char *const *argv, const char *out_path, const char *err_path, int device);
/* buffer level: reads as ASCII (seq_off has n+1 entries; qual NULL or parallel to seq, zero bytes = no qualities);
 * per read the masked bases (sdust_core, sdust.c:136-171), the sum of 10^(-q/10) over its qualities in read order
 * (meanQ = -10 log10(sum / length), lqutils.c:51-58) and getQV(qual, 7) (lqutils.c:61-69).  W in [3, 66].           */
int lqsdust_reads(int device, uint32_t n, const uint8_t *seq, const uint64_t *seq_off, const uint8_t *qual, int W, int T,
                  uint32_t *masked, double *qual_psum, uint32_t *n_above_q7, char *errbuf, size_t errbuf_len);

/* ---- the adapter search of sampleqc (lq_adapt.py:10-101, edlib.align(adapter, window, mode="HW", task="path")) ------ */
/* Reads as ASCII (seq_off has n+1 entries).  For every read of at least 2 * length bases, per adapter given (pointer not NULL,
 * length not 0), one row of four int32 in out5 / out3 [n x 4]: d (edit distance), s (start), e (first optimal end, -1 when
 * the whole adapter is deleted) and L (length of edlib's traceback path) of the adapter against the read's first (out5) or
 * last (out3) `length` bases, as edlib reports them; rows of shorter reads are -1.  The 3' row is that of the untrimmed read:
 * whether the reference skips it after a 5' trim is the caller's decision.  Bytes compare exactly.  length in [1, 4096],
 * adapters of at most 32768 bases (LQCOV_E_DOMAIN otherwise).                                                            */
int lqadapt_reads(int device, uint32_t n, const uint8_t *seq, const uint64_t *seq_off,
                  const uint8_t *adp5, uint32_t len5, const uint8_t *adp3, uint32_t len3,
                  uint32_t length, int32_t *out5, int32_t *out3, char *errbuf, size_t errbuf_len);

/* ---- the GC fraction step of sampleqc (lq_gcfrac.py:25-48, LqGC.calc_read_and_chunk_gc_frac) ------------------------- */
/* Reads as ASCII (seq_off has n+1 entries).  gc[i] = the number of 'G' and 'C' bytes of read i (no other byte counts).
 * k != NULL: read i has k[i] sampled positions (the caller computes int(1/chunk_size * l * samp_rate)), draw_off their n+1
 * prefix sums.  The positions are pos_in's, or -- pos_in == NULL -- drawn on the device: position j of read i is the image
 * of j under a bijection of [0, l) keyed by (seed, first_read + i), so the draw of a read depends on its
 * ordinal in the whole input alone; pos_out, if given, receives the positions used.  kept[i] = the index, in draw order, of
 * the first position p with p + chunk_size - 1 > l, where the reference's walk of the read ends, or k[i]; win_gc[d] = the
 * G/C bytes of seq[p : min(p + chunk_size, l)] for the draws before kept[i], 0 for the others.  All results are integers:
 * the fractions are the caller's divisions.  LQCOV_E_ARG: null buffers, offsets not ascending, draw_off not the prefix sums
 * of k, k[i] > l, a pos_in outside its read; LQCOV_E_DOMAIN: chunk_size outside [1, 4096], a read of 2^32 bases or more. */
int lqgc_reads(int device, uint32_t n, const uint8_t *seq, const uint64_t *seq_off,
               uint32_t chunk_size, const uint32_t *k, const uint64_t *draw_off, const uint32_t *pos_in,
               uint64_t seed, uint64_t first_read, uint32_t *gc, uint32_t *pos_out, uint16_t *win_gc, uint32_t *kept,
               char *errbuf, size_t errbuf_len);

/* ---- the numbers behind the GC figure and the length figure (lq_gcfrac.py:49-85, lq_gamma.py:47-59, longQC.py:487-488) ------------ */
/* Array-level calls over every read of a run; each uploads its array (fewer than 2^32 values, LQCOV_E_DOMAIN otherwise) and keeps
 * nothing resident.  dtype: the element type of x, float32 or uint32; every value is converted to double exactly.  LQCOV_E_ARG: null
 * pointers with non-zero sizes, another dtype, and what each call names.  Nothing is drawn.                                          */
#define LQFIG_F32 0
#define LQFIG_U32 1
/* *min_out / *max_out (4 bytes each, of x's type) = the smallest and largest value, NaN left out.  LQCOV_E_ARG: n == 0, or NaN alone. */
int lqfig_range(int device, int dtype, const void *x, uint64_t n, void *min_out, void *max_out, char *errbuf, size_t errbuf_len);
/* np.histogram(x, bins=edges)'s counts for an explicit edge array: counts[k], k < n_edges - 1, = the values with edges[k] <= v <
 * edges[k+1], the last bin closed on the right; a value below edges[0], above edges[n_edges-1] or NaN is counted nowhere.  n_edges < 2:
 * no bins, nothing written.  n == 0: zero counts.  LQCOV_E_ARG: edges not ascending (equal neighbours pass, as in numpy) or NaN.     */
int lqfig_hist(int device, int dtype, const void *x, uint64_t n, const double *edges, uint32_t n_edges, uint64_t *counts,
               char *errbuf, size_t errbuf_len);
/* sums[j], j < m, = sum over i < n of exp(-0.5 u u), u = (points[j] - data[i]) / h, in double, the difference taken first: the sum of
 * a Gaussian KDE before its normalisation (density = sums[j] / n / (h sqrt(2 pi))).  The terms are added in an order fixed by n alone
 * (tiles of 256 values in index order, a pairwise tree over the tiles): the same bytes from every call.  n == 0: zeros.
 * LQCOV_E_ARG: m == 0, h not finite or <= 0.                                                                                          */
int lqfig_kde(int device, const float *data, uint64_t n, const double *points, uint32_t m, double h, double *sums,
              char *errbuf, size_t errbuf_len);
/* *sum = sum of x (exact), *n_zero = the number of zeros, *sum_log = sum of log(x) over the non-zero values, in double, in the same fixed
 * order: what the gamma fit of the read lengths needs (mean and mean log).  n == 0: zeros.                                            */
int lqfig_logsum(int device, const uint32_t *x, uint64_t n, uint64_t *sum, double *sum_log, uint64_t *n_zero,
                 char *errbuf, size_t errbuf_len);
/* Box-plot statistics by group: what LongQC's grouped box plots compute before they draw (lq_mask.py:43-79, lq_coverage.py:438-529).
 * A value is a printed "%.3f" number as an integer count of thousandths, thou[i]; its double is thou / 1000 (one IEEE division, which is
 * float(text)); LQFIG_MISSING is "-nan".  The group of element i is key[i] when interval == 0, else floor((double)key[i] / interval), the
 * IEEE division (np.floor(len / interval)).  sorted (n entries) gets the values group by group, the groups ascending, inside a group the
 * non-missing values ascending and then the missing ones; boxes one entry per group that occurs, ascending in `group`: the group's
 * place in sorted[], and matplotlib.cbook.boxplot_stats(x, whis) of its non-missing values x -- q1, med, q3 by np.percentile's linear
 * rule, every operation rounded on its own; whishi the largest value <= q3 + whis (q3 - q1), or q3 if there is none or it lies below q3;
 * whislo its mirror; the fliers the n_low values below whislo and the n_high values above whishi, at the two ends of the group's stretch.
 * mid_lo / mid_hi: the two middle order statistics, for the median (a + b) / 2 of np.median and pandas.  A group without non-missing
 * values has NaN statistics, LQFIG_MISSING as both middles and no fliers.  The sort is on integers: the same bytes from every call.
 * n == 0: no boxes.  LQCOV_E_ARG: null buffers, interval or whis negative or not finite, box_cap smaller than the number of groups
 * -- *n_boxes is written all the same, and the next call works; LQCOV_E_DOMAIN: n >= 2^32, a group of 2^32 or more, a value of
 * INT32_MAX (its sort key is the missing value's).                                                                                      */
typedef struct lqfig_box {
	uint32_t group, reserved;
	uint64_t first, n_all, n;      /* place of the group in sorted[], its members, its non-missing members */
	int32_t  mid_lo, mid_hi;       /* the two middle order statistics, thousandths (equal for odd n) */
	double   q1, med, q3, whislo, whishi;
	uint64_t n_low, n_high;        /* fliers: sorted[first .. first+n_low) and sorted[first+n-n_high .. first+n) */
} lqfig_box;
#define LQFIG_MISSING INT32_MIN
int lqfig_boxstats(int device, const uint32_t *key, const int32_t *thou, uint64_t n, double interval, double whis,
                   int32_t *sorted, lqfig_box *boxes, uint32_t box_cap, uint32_t *n_boxes,
                   char *errbuf, size_t errbuf_len);

/* ---- the coverage estimate's two mixture fits (lq_coverage.py:552-621) ------------------------------------------------------------- */
/* n_fits independent fits in one launch, one workgroup per fit, the whole EM loop and its stopping rule on the device.  x: the fits'
 * values one after the other, off (n_fits + 1 ascending entries): fit f has x[off[f] .. off[f + 1]).  Every segment is sorted ascending
 * on the host first and every sum over it is added in an order fixed by its length alone (tiles of 256 values in index order, a pairwise
 * tree over the tiles): a fit is a function of its segment's values as a multiset -- the same bytes whatever the order of
 * the rows, the batch around it, the grid and the run.  LQCOV_E_ARG: null buffers, n_fits == 0, offsets not ascending, a segment of fewer
 * than 2 or more than LQMIX_MAX_N values, a value that is not finite, a segment whose values are all equal (no variance), and what
 * each call names.                                                                                                                      */
#define LQMIX_MAX_N 9216
#define LQMIX_EXIT_TOL 0           /* the stopping rule's tolerance was met */
#define LQMIX_EXIT_MAX 1           /* max_iter was reached */
#define LQMIX_EXIT_NAN 2           /* lqmix_lognorm: the log-likelihood became NaN; the numbers are reported as they are */
typedef struct lqmix_fit {
	double   w[2], mu[2];
	double   s[2];                 /* lqmix_gmm2: the variances; lqmix_lognorm: the sigmas */
	double   ll;                   /* lqmix_gmm2: the last lower bound; lqmix_lognorm: the last log-likelihood */
	uint32_t n_iter, exit;         /* E/M passes made (lqmix_lognorm: mixem's iteration + 1), LQMIX_EXIT_* */
	uint64_t n;                    /* the segment's size */
} lqmix_fit;
/* sklearn's GaussianMixture(n_components=2).fit of 1-D data after its initialisation (tol, max_iter, reg_covar: its 1e-3, 100, 1e-6),
 * from a deterministic start in place of its seeded k-means: the split of the sorted values into {first k} + {rest} with the smallest
 * two-cluster squared error (the smallest such k), as one-hot responsibilities.  The parameters are those after the M-step of the last
 * iteration; the components come out ascending in their mean.  tol < 0 never stops early.  LQCOV_E_ARG also for max_iter == 0, a
 * negative or non-finite reg_covar, a NaN tol.                                                                                          */
int lqmix_gmm2(int device, const double *x, const uint64_t *off, uint32_t n_fits, double tol, uint32_t max_iter, double reg_covar,
               lqmix_fit *out, char *errbuf, size_t errbuf_len);
/* mixem.em(data, [NormalDistribution(mu_bg, sigma_bg), LogNormalDistribution(mu_logn, sigma_logn)], max_iterations=max_iter, tol=tol,
 * tol_iters=tol_iters) (mixem's 1e-15 and 10; LongQC's max_iterations is 500): init has the four numbers of every fit; component 0 is
 * the normal, 1 the log-normal; initial weights (1, 1).  LQCOV_E_ARG also for a value <= 0, a sigma that is not positive and finite, a
 * mu that is not finite, tol_iters outside [1, 64], a NaN tol.                                                                          */
int lqmix_lognorm(int device, const double *x, const uint64_t *off, uint32_t n_fits, const double *init, double tol, uint32_t tol_iters,
                  uint32_t max_iter, lqmix_fit *out, char *errbuf, size_t errbuf_len);

/* ---- one upload per chunk: the chunk loop of sampleqc (longQC.py:299-360) and the coverage call on the same device bytes ---------- */
/* A resident chunk: lqchunk_load uploads the reads (ASCII, seq_off with n+1 ascending entries, qual NULL or parallel to seq as in
 * lqsdust_reads) once into device buffers the handle owns and reuses, growing, from chunk to chunk.  lqchunk_sdust, lqchunk_adapt and
 * lqchunk_gc are lqsdust_reads, lqadapt_reads and lqgc_reads on those buffers: the same arguments behind the reads, the same checks
 * and codes, the same results (those three are the same code on a chunk that lives for one call).  lqchunk_pack writes, on the device,
 * the packed form documented at lqcov_pack_reads, byte for byte what that call writes on the host, and per read the flag of
 * lqcov_packed_ambiguous_reads; lqchunk_get_packed copies the three arrays to the host (lqcov_packed_chunks(n, seq_off) chunks of 32
 * / 16 bytes, n flags).  A handle owns one stream and its calls are ordered on it; handles are not thread-safe.  LQCOV_E_STATE: no
 * chunk loaded, or not packed.  The message of a failed call is lqchunk_last_error's (c == NULL: why lqchunk_create failed). */
typedef struct lqchunk lqchunk;
lqchunk *lqchunk_create(int device);                 /* NULL without a HIP device */
void     lqchunk_destroy(lqchunk *c);
const char *lqchunk_last_error(const lqchunk *c);
int lqchunk_load(lqchunk *c, uint32_t n, const uint8_t *seq, const uint64_t *seq_off, const uint8_t *qual);
int lqchunk_sdust(lqchunk *c, int W, int T, uint32_t *masked, double *qual_psum, uint32_t *n_above_q7);
/* The same table with long reads cut into pieces that are scanned side by side (opt-in; k_sdust_pieces): a read of A/C/G/T alone (either
 * case) with at least two pieces' bases is cut into pieces of `piece` bases (0: the default, 4096), each scanned from empty state 2 W +
 * 2 bases before its first base, and what the pieces save is ORed into a bit mask of the read; every other read -- one with an N or
 * any other byte, one shorter than two pieces -- takes lqchunk_sdust's walk, a thread per read.  masked, qual_psum and n_above_q7 are
 * lqchunk_sdust's arrays, value for value; *n_serial (may be NULL) is the number of reads that took the serial walk.  The same checks
 * and codes as lqchunk_sdust; LQCOV_E_ARG also for 0 < piece < 2 W + 2.
 * lqchunk_sdust_intervals returns what the reference's library call sdust() returns for the reads the pieces serve: the maximal runs of
 * the mask, read i's in iv[n_off[i] .. n_off[i + 1]) as start << 32 | finish (ascending, disjoint, not adjacent, inside the read; the
 * sum of finish - start is masked[i]).  Here a read of any length is served, also one of a single piece; flagged[i] (n bytes, may be
 * NULL) is 1 for a read with a byte other than A/C/G/T, which only the serial walk can count: it reports no interval.  Two calls: with iv == NULL only n_off (n + 1 entries), flagged and *iv_need are written; with iv != NULL and iv_cap >=
 * *iv_need the intervals too (a smaller iv_cap: LQCOV_E_ARG).  The runs are taken from a copy of the mask on the host and kept for the
 * second call; every lqchunk_sdust_split call classifies and scans anew. */
int lqchunk_sdust_split(lqchunk *c, int W, int T, uint32_t piece, uint32_t *masked, double *qual_psum, uint32_t *n_above_q7, uint32_t *n_serial);
int lqchunk_sdust_intervals(lqchunk *c, int W, int T, uint32_t piece, uint64_t *n_off, uint8_t *flagged, uint64_t *iv, size_t iv_cap, size_t *iv_need);
/* The table as text, made on the device (opt-in; k_sdust_rows, k_sdust_patch, k_sdust_text): per read the row `sdust` prints,
 * name \t masked \t len \t %.3f of masked/len \t %.3f of meanQ \t q7 \n (sdust.c:211-217), byte for byte, one behind the other.
 * lqchunk_sdust and lqchunk_sdust_split take NULL for all three host arrays: the results then stay on the device.
 * lqchunk_sdust_table formats the results the chunk's last lqchunk_sdust / lqchunk_sdust_split left there: names / name_off as
 * lqstore_append takes them (NULL: empty names); out gets the text, out_cap is its room -- the sum of the names' lengths + 48 bytes per
 * read always suffices -- *out_len the text's length; stats (may be NULL) the table's summary; excl (may be NULL, else room for excl_cap
 * indices): the reads on LongQC's two exclusion lists (longQC.py:370-371, by the printed fraction: len > 500000 and more than 0.200, then
 * len > 10000 and more than 0.400), the first list's stats->excluded_first indices ascending, then the second's.
 * LQCOV_E_STATE: no chunk loaded, or no scan since the chunk was loaded; LQCOV_E_ARG: out_cap or excl_cap too small -- nothing is written
 * but *out_len and stats, and the next call works.
 * lqsdust_format is the same from arrays on the host: row i has masked[i], len[i], qual_psum[i], n_above_q7[i] and qualities if len[i] > 0
 * and has_q[i] != 0 (has_q NULL: no row has).  window: a row's meanQ is the device's unless |frac(|z| * 1000) - 0.5| < window * max(|z| *
 * 1000, 1), where the host takes it with libm; 0: the default, 2^-30; 1: every row with qualities.  stats->unvouched counts them.
 * lqsdust_format_lists is lqsdust_format with lqchunk_sdust_table's excl / excl_cap: the rows on the two exclusion lists. */
#define LQSDUST_STATS_WORDS 8
typedef struct lqsdust_stats {
	uint64_t rows, bytes;                /* rows and bytes of the text */
	uint64_t masked, q7;                 /* the sums of the two integer columns */
	uint64_t unvouched;                  /* rows whose meanQ the host took */
	uint64_t excluded, excluded_first;   /* entries of both exclusion lists, and of the first */
	uint64_t reserved;
} lqsdust_stats;
int lqchunk_sdust_table(lqchunk *c, const char *names, const uint64_t *name_off, uint8_t *out, uint64_t out_cap, uint64_t *out_len,
                        lqsdust_stats *stats, uint32_t *excl, uint64_t excl_cap);
int lqsdust_format(int device, uint32_t n, const char *names, const uint64_t *name_off, const uint32_t *masked, const uint32_t *len,
                   const double *qual_psum, const uint8_t *has_q, const uint32_t *n_above_q7, double window, uint8_t *out, uint64_t out_cap,
                   uint64_t *out_len, lqsdust_stats *stats, char *errbuf, size_t errbuf_len);
int lqsdust_format_lists(int device, uint32_t n, const char *names, const uint64_t *name_off, const uint32_t *masked, const uint32_t *len,
                         const double *qual_psum, const uint8_t *has_q, const uint32_t *n_above_q7, double window, uint8_t *out, uint64_t out_cap,
                         uint64_t *out_len, lqsdust_stats *stats, uint32_t *excl, uint64_t excl_cap, char *errbuf, size_t errbuf_len);
/* printf's "%.3f" as the table's kernels and the host take it (lq_fmt3.hpp): -> the class (0 finite, 1 nan, 2 inf, 3 2^50 or more; + 4:
 * the sign bit), *thousandths: |x| rounded to 1/1000 exactly, ties to even.  No device needed. */
uint32_t lqsdust_fmt3(double x, uint64_t *thousandths);
/* The two "%.3f" columns of the table lqchunk_sdust_table made last, as the thousandths its text shows (n entries each; the rows whose
 * meanQ the host took included: a row's numbers and its text never disagree): frac_thou[i] of masked/len, qv_thou[i] of meanQ, negative
 * where the text has a sign ("-0.000" is 0).  "-nan" is UINT32_MAX / LQFIG_MISSING.  LQCOV_E_STATE: no table of the chunk loaded now and of
 * its last scan (a lqchunk_sdust_table call that failed made none); LQCOV_E_DOMAIN: an infinite meanQ, or one of 2^31 - 1 thousandths or more. */
int lqchunk_sdust_columns(lqchunk *c, uint32_t *frac_thou, int32_t *qv_thou);
int lqchunk_adapt(lqchunk *c, const uint8_t *adp5, uint32_t len5, const uint8_t *adp3, uint32_t len3,
                  uint32_t length, int32_t *out5, int32_t *out3);
int lqchunk_gc(lqchunk *c, uint32_t chunk_size, const uint32_t *k, const uint64_t *draw_off, const uint32_t *pos_in,
               uint64_t seed, uint64_t first_read, uint32_t *gc, uint32_t *pos_out, uint16_t *win_gc, uint32_t *kept);
int lqchunk_pack(lqchunk *c);
int lqchunk_get_packed(lqchunk *c, uint64_t *codes, uint32_t *amb, uint8_t *amb_flags);

/* The packed chunks of a whole input, kept in device memory (0.25 B per base, 0.375 for a chunk with an ambiguous base; one
 * allocation per array and appended chunk), with lengths, names and flags on the host.  lqstore_append copies the packed form of a
 * chunk (after lqchunk_pack; names as in lqcov_set_queries, NULL: empty names) -- the chunk handle is free for the next chunk
 * afterwards.  If the device memory cannot be had the call fails with LQCOV_E_DEVICE (message on the chunk handle) and the store is
 * unchanged.  lqstore_run cuts the stored reads into index parts by the reference's rule (index.c:244,311-316, from the lengths
 * alone) and, part by part, fills a part of `h` from the stored chunks' pieces, builds, maps and releases it; the queries are those
 * set on `h`, lqcov_finish and the tables stay the caller's.  A failing engine call ends it with that call's code (lqcov_last_error). */
typedef struct lqstore lqstore;
lqstore *lqstore_create(int device);                 /* NULL without a HIP device */
void     lqstore_destroy(lqstore *s);
int      lqstore_append(lqstore *s, lqchunk *c, const char *names, const uint64_t *name_off);
uint64_t lqstore_bytes(const lqstore *s);            /* device bytes held */
int      lqstore_run(lqstore *s, lqcov_handle *h);

/* ---- the chunk loop's source: a plain or gzip FASTA/FASTQ file as resident chunks (lq_utils.py:263-289, parse_fastx_chunk) ---------- */
/* lqreader_next fills `c` (a handle of the reader's device) with the next chunk of the file: the records are kseq's (the name up to
 * the first whitespace, sequence lines concatenated, one trailing '\r' per line dropped, a truncated quality string ends the stream
 * after the records before it); a record without a quality string gets '!' for every base; is_upper turns a-z of the sequences into
 * A-Z on the device.  The chunk rule is the reference's: per record size += 3 * str_overhead + len(name) + 2 * len(seq)
 * (sys.getsizeof of the three str objects; str_overhead = sys.getsizeof("")), the chunk ends with the record that makes
 * size >= chunk_size.  *last = 1: the file has ended and this (possibly empty) chunk is the last one -- one such chunk always comes.
 * n_seqs_cum / n_bases_cum count the whole file so far.  The chunk is as after lqchunk_load (with qualities); lqreader_names points
 * at the names (NUL-terminated, name_off with n + 1 entries: the arguments of lqstore_append) and the lengths of the chunk made last,
 * valid until the next lqreader_next.  lqchunk_get_reads copies the bases (and, qual_out != NULL, the qualities) of the reads
 * idx[0 .. n_idx) -- idx == NULL: of all reads -- back to back to the host.  Errors: LQCOV_E_IO (the file cannot be opened: NULL from
 * lqreader_open, the message is lqreader_last_error(NULL)'s), LQCOV_E_DOMAIN (a name byte of 0x80 or more, a read of 2^31 bases),
 * LQCOV_E_STATE (lqreader_next after the last chunk).  n_threads <= 0: the default (at most 16). */
typedef struct lqreader lqreader;
lqreader *lqreader_open(const char *path, int device, uint64_t chunk_size, int is_upper, uint32_t str_overhead, int n_threads);
int  lqreader_next(lqreader *r, lqchunk *c, uint32_t *n, uint64_t *n_seqs_cum, uint64_t *n_bases_cum, int *last);
int  lqreader_names(const lqreader *r, const char **names, const uint64_t **name_off, const uint32_t **lens);
void lqreader_close(lqreader *r);
const char *lqreader_last_error(const lqreader *r);
/* An unaligned BAM file (a BGZF file whose inflated bytes begin with "BAM\1"; lq_utils.parse_bam_chunk) is read through the same
 * calls: lqreader_open recognises it, n_threads threads inflate its blocks, every record is a read whatever its flag, the name is
 * read_name, the sequence the decoded nibbles ("=ACMGRSVTWYHKDBN"; is_upper changes nothing).  lqreader_format: 0 FASTA/FASTQ, 1 BAM.
 * The qualities are '!' for every base, as open_seq_chunk's is_sequel=True gives them; lqreader_bam_qualities(r, 1) -- before the first
 * lqreader_next, LQCOV_E_STATE afterwards -- makes them chr(q + 33) of the file's (a record without qualities, first byte 0xff: '!').
 * On a FASTA/FASTQ reader the call changes nothing.  Errors: LQCOV_E_IO for a block cut short, a CRC32 or ISIZE mismatch, a record
 * whose block_size is too small for its fields, a name without its NUL, a file that ends inside a record. */
int  lqreader_format(const lqreader *r);
int  lqreader_bam_qualities(lqreader *r, int from_file);
/* The second way to inflate BGZF blocks, opt-in: lqreader_inflate(r, LQREADER_INFLATE_DEVICE) -- before the first lqreader_next,
 * LQCOV_E_STATE afterwards; the default is LQREADER_INFLATE_HOST, or what the environment variable LQREADER_INFLATE ("device") says
 * when the reader is opened -- has k_bgzf_inflate inflate them on the device: the compressed bytes go up, the inflated bytes come back
 * for the record walk and the CRC32 check (the pool's threads) and stay in the chunk's raw device buffer for the gather kernels, so
 * the piece is not uploaded.  The chunks, the errors (LQCOV_E_IO: "corrupt deflate stream", "ISIZE does not match the inflated
 * bytes", "CRC32 mismatch", the lowest failing file offset) are those of the host mode.  In device mode a BGZF file that is not BAM
 * (bgzip FASTA/FASTQ) is inflated the same way instead of by gzread; a gzip file that is not BGZF: below; any other file ignores the mode.
 * lqinflate_blocks is the array-level call (tests; callers that hold BGZF blocks of their own): block i is the raw deflate stream
 * comp[in_off[i] .. + in_len[i]) (in_len < 2^24) and inflates to out_host[out_off[i] .. + isize[i]), isize[i] <= 65536.  out_host[0 ..
 * max(out_off + isize)) goes to the device before the launch and comes back after it: bytes outside the blocks' ranges return as they
 * were given.  status[i]: 0 the stream ended after exactly isize bytes; LQINFLATE_INVALID not a deflate stream; LQINFLATE_INPUT the input
 * ended inside the stream; LQINFLATE_LONG / LQINFLATE_SHORT a valid stream of more / fewer bytes (what a failing block leaves in its
 * range is unspecified, nothing outside it is written).  A bad block is not an error of the call.  LQCOV_E_ARG: null buffers, a range
 * outside comp, isize above 65536 (the message: lqreader_last_error(NULL)). */
#define LQREADER_INFLATE_HOST   0
#define LQREADER_INFLATE_DEVICE 1
#define LQINFLATE_INVALID 1
#define LQINFLATE_INPUT   2
#define LQINFLATE_LONG    3
#define LQINFLATE_SHORT   4
int  lqreader_inflate(lqreader *r, int mode);
int  lqinflate_blocks(int device, const uint8_t *comp, uint64_t comp_len, uint32_t n, const uint64_t *in_off, const uint32_t *in_len,
                      const uint64_t *out_off, const uint32_t *isize, uint8_t *out_host, uint32_t *status);
/* A gzip file that is not BGZF (what gzip, pigz and most sequencers' pipelines write) carries no block sizes; in device mode it is
 * inflated by speculative spans: the compressed bytes are cut into spans of LQREADER_GZ_SPAN_BYTES (environment,
 * read when the reader starts; default 16384, at least 1024, at most 131072, a multiple of 16), k_gz_find looks in each for a
 * dynamic block's header, k_gz_inflate_spec decodes every span without its history, and a span counts only if it starts at the bit
 * where the span before it ended (the chain).  What the device cannot vouch for -- an error, a block that fits no span's region -- zlib
 * redoes on the host from the last accepted block boundary, and zlib's verdict is the call's.  Chunks, borders, counts and names are
 * the host mode's, and so is the one error: LQCOV_E_IO, "failed to open file '...': not a complete gzip stream" (a bad header, a
 * corrupt block, a wrong CRC32 or ISIZE; as with gzread, a file that merely ends early ends the reads, and bytes behind the last
 * member that are not a gzip header are ignored).  How many chunks come out before that error is not part of the contract.
 * lqreader_inflate_stats: what the reader's gzip stream has done so far (zeros for any other file or mode).
 * lqinflate_gzip is the array-level call: comp[0 .. comp_len) is a whole gzip file, its bytes go to out[0 .. *out_len), *out_len <=
 * out_cap (LQCOV_E_ARG if the stream is longer); span_bytes: 0 the default, else as LQREADER_GZ_SPAN_BYTES; stats may be NULL. */
typedef struct lqinflate_stats {
	uint64_t launches;           /* windows of compressed bytes uploaded and decoded */
	uint64_t spans_found;        /* spans in which the search found a block header (a launch's first span is given, not found) */
	uint64_t spans_accepted;     /* of those: accepted by the chain */
	uint64_t spans_rejected;     /* of those: not accepted -- the span at which the chain broke and every span behind it in that launch */
	uint64_t markers_resolved;   /* symbols that stood for a byte in front of their span */
	uint64_t bytes_device;       /* inflated bytes the device made */
	uint64_t bytes_zlib;         /* inflated bytes zlib made on the host instead */
} lqinflate_stats;
int  lqreader_inflate_stats(const lqreader *r, lqinflate_stats *stats);
int  lqinflate_gzip(int device, const uint8_t *comp, uint64_t comp_len, uint32_t span_bytes, uint8_t *out, uint64_t out_cap, uint64_t *out_len,
                    lqinflate_stats *stats);
/* The record scan on the device, opt-in: lqreader_parse(r, LQREADER_PARSE_DEVICE) -- before the first lqreader_next,
 * LQCOV_E_STATE afterwards; the default is LQREADER_PARSE_HOST, or what the environment variable LQREADER_PARSE ("device") says when
 * the reader is opened; a BAM reader accepts the mode and ignores it (its switch is lqreader_bam_walk, below).  Every piece of the file is then uploaded as it is read (with
 * lqreader_inflate's device mode it is there already), k_fx_* find the records of the piece there and write the segment lists that
 * k_chunk_gather reads; the host gets 16 bytes per record (where the name is, its length, the sequence's length, whether there is a
 * quality string), copies the names out of the piece and applies the chunk rule.  The device answers only for records it can vouch
 * for: the header character is a line's first byte, no sequence or quality line is exactly "\r" and no empty line follows one that
 * ends in "\r\r", the record is complete inside the piece whatever follows it (FASTQ: the quality string reaches the sequence's
 * length exactly, at the end of a line that has its line break; FASTA: the next header's first byte is there), fewer than 2^31
 * bases.  Every other record, and everything at the end of the file, is the host parser's as before; chunks, borders, counts,
 * names and errors are the host mode's.  lqreader_parse_stats says what happened so far.
 * lqfx_scan is the array-level call: bytes[0 .. n) on the host, a parser that stands at start_pos with kseq's last_char (0, '@' or
 * '>': that header character is bytes[start_pos - 1]).  rows: 4 words per vouched record (name offset, name length, sequence
 * length, flags: bit 0 a quality string), sseg / qseg: (src, dst) pairs as k_chunk_gather takes them, src an offset into bytes (or
 * all ones: no quality string, '!'), dst the place in the concatenated sequences of the vouched records.  The vouched records are
 * the first *n_rows records kseq reads from that state; (*resume_pos, *resume_last_char) is the state behind them.  A start that is
 * not a line's first byte gives no rows.  LQCOV_E_ARG: null buffers, tables smaller than the result, a last_char that bytes does not
 * hold (the message: lqreader_last_error(NULL)). */
#define LQREADER_PARSE_HOST   0
#define LQREADER_PARSE_DEVICE 1
typedef struct lqparse_stats {
	uint64_t pieces;             /* reads of the file that brought bytes */
	uint64_t scans;              /* scans run on the device */
	uint64_t records_device;     /* records the device vouched for */
	uint64_t records_host;       /* records the host parser made */
	uint64_t lines;              /* lines the scans saw */
	uint64_t fallbacks;          /* scans that stopped in front of a complete record of their range */
} lqparse_stats;
int  lqreader_parse(lqreader *r, int mode);
int  lqreader_parse_stats(const lqreader *r, lqparse_stats *stats);
int  lqfx_scan(int device, const uint8_t *bytes, uint64_t n, uint64_t start_pos, int last_char, uint32_t *rows, uint64_t n_rows_cap,
               uint64_t *sseg, uint64_t *qseg, uint64_t seg_cap, uint64_t *n_rows, uint64_t *n_sseg, uint64_t *n_qseg,
               uint64_t *resume_pos, int *resume_last_char);
/* Inflated bytes that stay on the device, opt-in: lqreader_host_copy(r, LQREADER_HOSTCOPY_NEEDED) -- before the first
 * lqreader_next, LQCOV_E_STATE afterwards; the default is LQREADER_HOSTCOPY_ALL, or what the environment variable LQREADER_HOSTCOPY
 * ("needed") says when the reader is opened.  The mode is active for a FASTA/FASTQ file that the device both inflates and parses
 * (lqreader_inflate and lqreader_parse in their device modes, a BGZF or gzip file) and for a BAM file that the device both inflates
 * and walks (lqreader_inflate and lqreader_bam_walk in their device modes); any other reader accepts it and ignores it.
 * When it is active the inflated bytes are not copied back: k_crc32_ranges makes every member's CRC32 from the chunk's raw device
 * buffer (BGZF: one value per block; gzip spans: the bytes a launch accepted, folded into the member's value by length; what zlib
 * inflates on the host is checked there as before), k_fx_names gathers the names of the records the device vouches for, and the
 * host fetches only what its own parser has to look at: the bytes from the parser's position to the end of the piece, when the
 * scan stops in front of them.  Chunks, borders, counts, names, statistics and errors are those of LQREADER_HOSTCOPY_ALL.
 * lqreader_copy_stats says what moved.
 * lqcrc32_ranges is the array-level call of k_crc32_ranges: crc_out[i] = zlib's crc32(0, bytes + off[i], len[i]) for i < n, 0 for an
 * empty range; the ranges may touch or overlap.  LQCOV_E_ARG: null buffers, a range outside [0, n_bytes).
 * lqfx_names is the array-level call of k_fx_names: rows as lqfx_scan writes them (4 words per row; the name of row i is
 * bytes[rows[4 i] .. + rows[4 i + 1])); names_out gets every name followed by one NUL, name_off_out the n_rows + 1 offsets, *first_bad
 * the first row whose name holds a byte of 0x80 or more (n_rows: none).  LQCOV_E_ARG: null buffers, a name outside bytes, names_cap
 * smaller than the blob.  The message of both: lqreader_last_error(NULL). */
#define LQREADER_HOSTCOPY_ALL    0
#define LQREADER_HOSTCOPY_NEEDED 1
typedef struct lqcopy_stats {
	uint64_t active;             /* 1: the mode is LQREADER_HOSTCOPY_NEEDED and this reader can honour it */
	uint64_t bytes_inflated;     /* inflated bytes of the file so far (device inflate only) */
	uint64_t bytes_to_host;      /* of those: copied from the raw device buffer into the piece (rows and names are not counted) */
	uint64_t bytes_crc_device;   /* bytes whose CRC32 k_crc32_ranges made */
	uint64_t bytes_crc_host;     /* bytes whose CRC32 zlib made on the host */
	uint64_t names_device;       /* names that came from k_fx_names */
} lqcopy_stats;
int  lqreader_host_copy(lqreader *r, int mode);
int  lqreader_copy_stats(const lqreader *r, lqcopy_stats *stats);
int  lqcrc32_ranges(int device, const uint8_t *bytes, uint64_t n_bytes, uint32_t n, const uint64_t *off, const uint64_t *len, uint32_t *crc_out);
int  lqfx_names(int device, const uint8_t *bytes, uint64_t n, const uint32_t *rows, uint64_t n_rows, char *names_out, uint64_t names_cap,
                uint64_t *name_off_out, uint64_t *first_bad);
/* The record walk of an unaligned BAM on the device, opt-in: lqreader_bam_walk(r, LQREADER_BAMWALK_DEVICE) -- before
 * the first lqreader_next, LQCOV_E_STATE afterwards; the default is LQREADER_BAMWALK_HOST, or what the environment variable
 * LQREADER_BAMWALK ("device") says when the reader is opened; a FASTA/FASTQ reader accepts the mode and ignores it.  Every piece of
 * inflated bytes is then on the device as it comes (uploaded, or with lqreader_inflate's device mode there already), k_bam_* find
 * the records of the piece there and write the segment lists that k_bam_gather / k_bam_qual read; the host gets 16 bytes per record
 * and applies the chunk rule.  The device answers only for records it can vouch for: offset o of a piece of n bytes is vouched iff
 * o + 36 <= n, refID = pos = next_refID = next_pos = -1 (bytes o+4 .. o+11 and o+24 .. o+31 are 0xff), l_read_name >= 1, l_seq and
 * block_size <= 2^31 - 1, block_size >= 32 + l_read_name + 4 n_cigar_op + (l_seq + 1) / 2 + l_seq, o + 4 + block_size <= n and the
 * byte o + 36 + l_read_name - 1 is 0; the records it reports are the longest run of vouched offsets of the chain start, next(start),
 * .. with next(o) = o + 4 + block_size.  Everything else -- the BAM header, aligned records, broken records, the record that
 * straddles the piece's end, the end of the file -- is the host walk's as before; chunks, borders, counts, names and errors are the
 * host walk's.  lqreader_parse_stats reports for it in the same fields (lines: the candidates the scans examined).  With
 * lqreader_inflate's device mode as well, lqreader_host_copy(r, LQREADER_HOSTCOPY_NEEDED) is active for the BAM: the blocks' CRC32 and
 * the names are made on the device, the host fetches what the header and its own walk look at.
 * lqbam_scan is the array-level call: bytes[0 .. n) on the host, the inflated bytes of a piece, a parser that stands at start_pos, a
 * record boundary behind the BAM header.  rows, sseg, qseg, the counts and the errors are lqfx_scan's (rows: name offset, strlen of
 * the name, l_seq, flags: bit 0 with_qual; one sseg per record with bases, src the first byte of the packed sequence; one qseg, src
 * the first quality byte with with_qual, else all ones); lqfx_names accepts the rows.  *resume_pos: the first offset of the chain
 * that is not vouched, or n. */
#define LQREADER_BAMWALK_HOST   0
#define LQREADER_BAMWALK_DEVICE 1
int  lqreader_bam_walk(lqreader *r, int mode);
int  lqbam_scan(int device, const uint8_t *bytes, uint64_t n, uint64_t start_pos, int with_qual, uint32_t *rows, uint64_t n_rows_cap,
                uint64_t *sseg, uint64_t *qseg, uint64_t seg_cap, uint64_t *n_rows, uint64_t *n_sseg, uint64_t *n_qseg,
                uint64_t *resume_pos);
int  lqchunk_get_reads(lqchunk *c, uint32_t n_idx, const uint32_t *idx, uint8_t *seq_out, uint8_t *qual_out);

/* ---- the chunk loop's files: trimmed reads (longQC.py:345-346) and the FASTQ a BAM file is converted to (:302-303) ------------------ */
/* The reads of a resident chunk as FASTQ text, made on the device (k_fastq_format): record i is '@' name '\n' seq[begin[i]:end[i]]
 * '\n' '+' '\n' qual[begin[i]:end[i]] '\n' -- what lq_utils.write_fastq writes for the record cut that way.  names / name_off: as
 * lqstore_append takes them (NUL-terminated, n offsets; names == NULL: empty names); begin == end == NULL: whole reads.
 * lqchunk_fastq makes the whole text in out[0 .. *out_len) (*out_len is set to the text's length also when out_cap is too small).
 * lqfastq_* streams it into a file: lqfastq_write makes the text in pieces of piece_bytes (a multiple of 4096, 0: the default of 16
 * MiB; byte ranges of the text, not records), each copied into one of two page-locked buffers on the chunk's stream and appended to
 * the file by the writer's thread while the next piece is made; it returns when the last piece is in its buffer -- the chunk handle is
 * free for the next chunk -- with *bytes_written the text's length (bytes_written may be NULL).  The file is opened for appending
 * (created if missing) when the first byte comes; a chunk without reads writes nothing and creates nothing.  lqfastq_close waits for
 * the thread, closes the file, frees the writer and returns its first error; the file is complete when it returns 0.
 * Errors: LQCOV_E_ARG -- begin[i] > end[i], end[i] > the read's length, a chunk loaded without qualities, a chunk of another device,
 * out_cap too small (nothing was written, the writer stays usable); LQCOV_E_STATE -- no chunk loaded; LQCOV_E_IO -- the file cannot
 * be opened or written (from the lqfastq_write that meets it, a later one, or lqfastq_close); LQCOV_E_DEVICE.  After an I/O or device
 * error every later lqfastq_write returns that error at once.  The message: lqchunk_last_error (lqchunk_fastq), lqfastq_last_error(w),
 * and lqfastq_last_error(NULL) for a failed lqfastq_open and for what lqfastq_close reported (per thread).  lqfastq_kernel_ms:
 * k_fastq_format's time on the device over all writes so far (HIP events), for measurements. */
typedef struct lqfastq lqfastq;
int  lqchunk_fastq(lqchunk *c, const char *names, const uint64_t *name_off, const uint32_t *begin, const uint32_t *end,
                   uint8_t *out, uint64_t out_cap, uint64_t *out_len);
lqfastq *lqfastq_open(const char *path, int device, uint64_t piece_bytes);
int  lqfastq_write(lqfastq *w, lqchunk *c, const char *names, const uint64_t *name_off, const uint32_t *begin, const uint32_t *end,
                   uint64_t *bytes_written);
int  lqfastq_close(lqfastq *w);
const char *lqfastq_last_error(const lqfastq *w);
double lqfastq_kernel_ms(const lqfastq *w);

/* ---- Sequel platform QC: the polymerase reads of a run from *.scraps.bam and *.subreads.bam (lq_sequel.run_platformqc) ------------- */
/* A handle collects items (zmw, start, end, class) on the device, 16 bytes each, and lqpol_finish makes of them what
 * lq_sequel.py:260-336 makes of its dict: per ZMW construct_polread's hq, tot, is_pol and ad_num, and over the ZMWs with is_pol the
 * sums, N50 and N90.  kind: 0 the scraps file, 1 the subreads file; every scraps item arrives before every subreads
 * item (scraps after subreads: LQCOV_E_STATE), and within a ZMW items with equal (start, end) keep their arrival order.
 * lqpol_add_bytes: bytes[0 .. n) on the host, inflated BAM bytes, a parser that stands at start_pos, a record boundary behind the BAM
 * header; the records that are whole are taken, *resume_pos is the first byte of the one that is not (or n), as lqbam_scan's.  The
 * device walk (k_bam_*) finds the records it vouches for, k_pol_fields reads their names and -- in the scraps file -- their sz and sc
 * tags; a record outside its domain (name not "x/zmw/start_end" with zmw, start, end of 1 to 9 digits and zmw without leading zeros;
 * an sz or sc that is not of type A; a tag area that does not end at the record's end) and a record the walk does not vouch for are
 * read by the host instead, which fails with LQCOV_E_IO where lq_sequel.py would raise and with LQCOV_E_DOMAIN where a value does
 * not fit an item; the message names the record.
 * lqpol_add_file: the whole BAM file in pieces; inflate_mode LQREADER_INFLATE_*, host_copy_mode LQREADER_HOSTCOPY_*: with the device's
 * inflate and LQREADER_HOSTCOPY_NEEDED the inflated bytes stay on the device (the blocks' CRC32 is made there) and the host fetches the
 * BAM header, 36 bytes of the record that straddles a piece's end, the records it has to read itself and, for a scan with a flagged
 * record, that scan's flags and rows (20 bytes a record).  lqpol_header_text: the header text of the file added last for `kind` (*len
 * its length, at most cap bytes copied); lqpol_file_header: the same of a file, read from its first blocks alone, without a handle --
 * for a caller that checks the header before it reads on.
 * lqpol_add_items: items given directly (cls: the class letter), in any state before lqpol_finish.
 * lqpol_finish: once; *control the control throughput.  lqpol_get: the per-ZMW arrays (n_zmw entries, ascending zmw; NULL: not wanted).
 * lqpol_stats: LQPOL_STATS_WORDS words -- sum of hq, max hq, min tot, max tot, N50, N90, the is_pol ZMWs with tot == 0 (the reference
 * divides by it), min and max ad_num, all over the is_pol ZMWs; the ZMWs the second walk launch took; records read by k_pol_fields,
 * re-read by the host because flagged, walked by the host; inflated bytes, bytes fetched to the host, pieces; the is_pol ZMWs whose hq or
 * tot is negative or above 2^32-1 (with any, the sums are void and lqpol_hist / lqpol_logsum return LQCOV_E_DOMAIN).
 * lqpol_hist / lqpol_logsum: lqfig_hist / lqfig_logsum over the resident uint32 array `which` of the is_pol ZMWs (logsum: LQPOL_HQ).
 * lqpol_fields / lqpol_twin: the two readers of a record alone, for tests -- the device's flags (bit 0 item, bit 1 flagged, bit 2
 * control) and compacted slots (16 bytes each; a flagged record's slot holds zmw 0x7fffffff) over the vouched records of a range, and
 * the host's reading of one whole record. */
typedef struct lqpol lqpol;
#define LQPOL_STATS_WORDS 17
#define LQPOL_HQ  0
#define LQPOL_TOT 1
#define LQPOL_AD  2
lqpol *lqpol_create(int device);                     /* NULL without a HIP device */
void   lqpol_destroy(lqpol *p);
const char *lqpol_last_error(const lqpol *p);
int lqpol_add_bytes(lqpol *p, int kind, const uint8_t *bytes, uint64_t n, uint64_t start_pos, uint64_t *resume_pos);
int lqpol_add_file(lqpol *p, int kind, const char *path, int inflate_mode, int host_copy_mode);
int lqpol_header_text(const lqpol *p, int kind, char *buf, uint64_t cap, uint64_t *len);
int lqpol_file_header(const char *path, char *buf, uint64_t cap, uint64_t *len, char *errbuf, size_t errbuf_len);
int lqpol_add_items(lqpol *p, const uint32_t *zmw, const uint32_t *start, const uint32_t *end, const uint8_t *cls, uint64_t n);
int lqpol_finish(lqpol *p, uint64_t *n_zmw, uint64_t *n_pol, int64_t *control);
int lqpol_get(lqpol *p, uint32_t *zmw, int64_t *hq, int64_t *tot, uint32_t *ad, uint8_t *is_pol);
int lqpol_stats(const lqpol *p, uint64_t out[LQPOL_STATS_WORDS]);
int lqpol_hist(lqpol *p, int which, const double *edges, uint32_t n_edges, uint64_t *counts);
int lqpol_logsum(lqpol *p, uint64_t *sum, double *sum_log, uint64_t *n_zero);
int lqpol_fields(int device, int kind, const uint8_t *bytes, uint64_t n, uint64_t start_pos, uint32_t *flags, uint32_t *items, uint64_t cap,
                 uint64_t *n_rows, uint64_t *n_slots, int64_t *control, uint64_t *resume_pos, char *errbuf, size_t errbuf_len);
int lqpol_twin(int kind, const uint8_t *rec, uint64_t len, uint64_t rec_no, uint32_t item[4], int64_t *control, uint32_t *flags,
               char *errbuf, size_t errbuf_len);

/* ---- box-plot statistics by group over doubles (df.boxplot(column=..., by=...), lq_rs.py:17-19) -------------------------------------- */
/* lqfig_boxstats on values that are doubles already: the same groups (key[i], or floor((double)key[i] / interval)), the same
 * matplotlib.cbook.boxplot_stats(x, whis) per group, every operation rounded on its own.  The values are ordered by their sign-corrected
 * bit pattern (-0.0 in front of +0.0) with two stable radix passes, by value and then by group.  There is no missing value: n == n_all.
 * LQCOV_E_DOMAIN also for a NaN.                                                                                                        */
typedef struct lqfig_box_f64 {
	uint32_t group, reserved;
	uint64_t first, n_all, n;
	double   mid_lo, mid_hi;       /* the two middle order statistics (equal for odd n) */
	double   q1, med, q3, whislo, whishi;
	uint64_t n_low, n_high;
} lqfig_box_f64;
int lqfig_boxstats_f64(int device, const uint32_t *key, const double *x, uint64_t n, double interval, double whis,
                       double *sorted, lqfig_box_f64 *boxes, uint32_t box_cap, uint32_t *n_boxes,
                       char *errbuf, size_t errbuf_len);

/* ---- a comma-separated table read into typed columns on the device; RS-II platform QC (lq_rs.run_platformqc) ------------------------ */
/* The domain: one header line, ',' as the separator, no '"' anywhere, every data row with the header's field count,
 * lines ending in "\n" or "\r\n" (a last line without either is a row), empty lines skipped.  lqcsv_want names a header column to read
 * and its kind before any byte arrives (at most 16; of a repeated header name the first column counts); column numbers in the later
 * calls are the order of the lqcsv_want calls.  An LQCSV_INT64 field is "[+-]?[0-9]{1,18}".  An LQCSV_DOUBLE field of at most 15
 * significant digits and 22 decimals, without exponent, is read by the device as one IEEE division of its integer mantissa by an exact
 * power of ten, which is the correctly rounded double; any other number is read by the host with strtod in the C locale.  Everything
 * else -- a quote, NUL, a lone '\r', a ragged row, a missing wanted column, an empty field, text, nan, inf or 19 digits in a wanted
 * column -- is LQCOV_E_DOMAIN with the line number and the reason; unwanted columns may hold any text.
 * lqcsv_add_bytes: bytes[0 .. n) of the file, behind what earlier calls consumed; whole lines are taken, piece by piece, *resume is the
 * first byte of the line that is not whole (the caller passes it again); with last != 0 that line is a row.  lqcsv_add_file: the whole
 * file, read and uploaded piece by piece.  lqcsv_set_piece_bytes: the size of a piece (tests; 0: the default, 8 MiB).
 * lqcsv_get: column col, n_rows int64 or double values.  lqcsv_stats: rows, fields parsed on the device, fields read by the host twin,
 * pieces, bytes.
 * lqcsv_lengths (after lqcsv_finish), on the resident columns: len = end_col - start_col per row (int64 columns; a value outside
 * 0 .. 2^32-1 in any row: LQCOV_E_DOMAIN), the mask score_col > threshold (a double column), and under the mask the compacted len
 * (LQCSV_HQ) and bases_col (LQCSV_BASES, int64, 0 .. 2^32-1), their sums, minima and maxima, and N50 / N90 of len by get_N50 / get_NXX's
 * rule (lq_utils.py:33-53).  out: masked rows, sum / min / max of len, N50, N90, sum / min / max of the bases, 0.
 * lqcsv_get_lengths / lqcsv_hist / lqcsv_logsum: the uint32 array `which` -- LQCSV_HQ, LQCSV_BASES (masked rows), LQCSV_LEN_ALL (every
 * row) -- fetched, or under lqfig_hist / lqfig_logsum (logsum: LQCSV_HQ).
 * lqcsv_boxstats: lqfig_boxstats_f64 with key = len of every row and x = the double column value_col, both where they lie.           */
typedef struct lqcsv lqcsv;
#define LQCSV_INT64  0
#define LQCSV_DOUBLE 1
#define LQCSV_STATS_WORDS 5
#define LQCSV_LEN_WORDS 10
#define LQCSV_HQ      0
#define LQCSV_BASES   1
#define LQCSV_LEN_ALL 2
lqcsv *lqcsv_create(int device);                     /* NULL without a HIP device */
void   lqcsv_destroy(lqcsv *p);
const char *lqcsv_last_error(const lqcsv *p);
int lqcsv_want(lqcsv *p, const char *name, int kind);
int lqcsv_set_piece_bytes(lqcsv *p, uint64_t bytes);
int lqcsv_add_bytes(lqcsv *p, const uint8_t *bytes, uint64_t n, int last, uint64_t *resume);
int lqcsv_add_file(lqcsv *p, const char *path);
int lqcsv_finish(lqcsv *p, uint64_t *n_rows);
int lqcsv_get(lqcsv *p, uint32_t col, void *out);
int lqcsv_stats(const lqcsv *p, uint64_t out[LQCSV_STATS_WORDS]);
int lqcsv_lengths(lqcsv *p, uint32_t score_col, double threshold, uint32_t start_col, uint32_t end_col, uint32_t bases_col,
                  uint64_t out[LQCSV_LEN_WORDS]);
int lqcsv_get_lengths(lqcsv *p, int which, uint32_t *out);
int lqcsv_hist(lqcsv *p, int which, const double *edges, uint32_t n_edges, uint64_t *counts);
int lqcsv_logsum(lqcsv *p, uint64_t *sum, double *sum_log, uint64_t *n_zero);
int lqcsv_boxstats(lqcsv *p, uint32_t value_col, double interval, double whis, double *sorted, lqfig_box_f64 *boxes, uint32_t box_cap,
                   uint32_t *n_boxes);

#ifdef __cplusplus
}
#endif
#endif
