// longqc_amd/csrc/engine.hpp -- host-side orchestration of the MI355X coverage engine.
//
// Mirrors the structure of the reference's main (minimap2-coverage.c:206-734): query set once
// (pass 1, :406-444), then per index part: build (index.c:311-330) + mid_occ on the first part
// (map.c:46-54) + map every query (lqmap.c:852 -> :207-326), then pass 2 (:545-617).  All state
// that the reference keeps per query on the host (lambdas, lambdas2, avg_ks, m_cnts, ovlp_coords)
// lives in HBM here; the host sees it only in finish().
#pragma once
#include "lq_common.hpp"
#include "prim.hpp"
struct KeyMap;
struct PsData;
struct AvaView;
struct EmitSub;
struct SeedGeometry;
struct SeedChunk;
struct SeedRun;
#include "../../include/lqcov.h"
#include <string>
#include <vector>
#include <map>
#include <memory>
#include <mutex>
#include <condition_variable>
#include <thread>
#include <atomic>
#include <exception>

struct StageAcc { double ms = 0; u64 launches = 0; u64 bytes = 0; };

// Environment switches, read once when the handle is made (test and A/B aids; the defaults are the measured choice).
struct Knobs {
	int lanes = 3;                        // LQCOV_LANES: concurrent mapping lanes (round 4, configs[2], ms per step: 2 lanes 908, 3: 888-922, 4: 964, 5: 995; round 3, every hit sorted: 1 lane 1882, 3: 1582, 5: 1510, 8: 1610)
	u64 anchor_budget = 0;                // LQCOV_ANCHOR_BUDGET: anchors per query batch (0 = from free HBM)
	bool query_order_striped = false;     // LQCOV_QUERY_ORDER=striped: longest first, then dealt to the lanes' stripes (round 6: measured, no gain)
	bool query_order_file = false;        // LQCOV_QUERY_ORDER=file: keep the caller's query order inside
	bool all_klib = false;                // LQCOV_SORT=klib: every query through klib's passes, no bucket leaves them early
	u32 ps_shift = 0;                     // LQCOV_PS_SHIFT: shrinks the size classes of the parallel sort (tests)
	bool reg_walker = true;               // LQCOV_WALK=solo: no register-lane walker
	bool ckpt = true, ckpt3 = true;       // LQCOV_CKPT=0: no checkpointed walks; LQCOV_CKPT3=0: the 65-160 k class is walked whole
	u32 sort_tile = 0;                    // LQCOV_SORT_TILE: anchors per tile of the sort's streaming kernels (0 = LQ_SORT_TILE)
	u32 walk_shift = 0;                   // LQCOV_WALK_SHIFT: shrinks the walker size classes and the checkpoint spacing (tests)
	int chain_wave_min = 0, chain_cap = 128;   // LQCOV_CHAIN_WAVE_MIN (0 = LQ_CHAIN_WAVE_MIN), LQCOV_CHAIN_CAP
	bool sketch_fast = true;              // LQCOV_SKETCH_FAST=0: k_sketch_dp_mask although k_sketch_dp_fast applies (-k 12 with -w 5 or 10; tests, A/B)
	bool upload_amb = false;              // LQCOV_UPLOAD_AMB=1: lqcov_run_files uploads the ambiguity words of a part although none of its reads holds an ambiguous base (rounds 2-5)
	bool sketch_wgen = false;             // LQCOV_SKETCH_WGEN=1: k_sketch_dp_mask with the window read at run time although it is 5 or 10 (tests, A/B)
	bool ps_key64 = false;                // LQCOV_PS_KEY64=1: the finishing kernels' 64-bit key shape although 32 bits would do (tests: parts with more than 2^40 (target, position) pairs are out of their reach)
	u32 run_grid = 2048;                  // LQCOV_RUN_GRID: blocks of k_run_list, each with a contiguous stretch of tiles (tests: 1 or 2, so that a block walks many)
	u32 run_stage = 2048;                 // LQCOV_RUN_STAGE: entries of the run list a block collects before it reserves their place (tests shrink it)
	bool no_level_skip = false;           // LQCOV_NO_LEVEL_SKIP: constant key bytes are walked, not stepped over
	bool debug_sort = false;              // LQCOV_DEBUG_SORT
	u32 sketch_kpt = 4;                   // LQCOV_SKETCH_KPT: chunks per thread of the sketch state machine
	u32 ps_passes = 2;                    // LQCOV_PS_PASSES: partition passes issued without looking (even; the tail looks at the counter and does the rest).  Two cover queries of up to ~500 M anchors against 65 536 targets; measured 4 vs 2 at configs[2]: 1.71-1.77 vs 1.69-1.71 s per step
	u32 tile_grid = 4096;                 // LQCOV_TILE_GRID: blocks of klib's tile kernels (histogram, scatter)
	u64 upload_min_chunks = 1u << 16;     // LQCOV_UPLOAD_MIN_CHUNKS: only read sets of that many 128-base chunks go up in slices (tests lower it)
	u32 upload_slices = 4;                // LQCOV_UPLOAD_SLICES (1..8): packed reads go up in slices, the data-parallel sketch kernel takes a slice while the next one is on its way (1: one copy, then the sketch)
	bool sketch_machine_only = false;     // LQCOV_SKETCH=machine: the state machine decides every chunk (no data-parallel kernel)
	bool ties_klib = false;               // LQCOV_TIES=klib (or LQCOV_SORT=klib): klib's order of equal-x anchors everywhere, every seed hit written and sorted (rounds 1-3); default: only where it can be observed (map_batch)
	bool filter = true;                   // LQCOV_FILTER=0: the first pass writes every seed hit (no counting filter)
	bool plan_ahead = true;               // LQCOV_PLAN_AHEAD=0: a part's seed plan (probe, survivors) is made when the part is mapped, not right after its index
	int parse_threads = 0;                // LQCOV_PARSE_THREADS: threads that parse and pack a plain target file (0: one per core, at most 64; 1: the streaming reader as for gzip)
	u64 parse_piece = 32u << 20;          // LQCOV_PARSE_PIECE: bytes of the file a thread parses at a time (tests shrink it: many guessed record starts)
	u64 parse_side = 2ULL << 30;          // LQCOV_PARSE_SIDE: bytes of multi-line records the mapped reader may copy before run_files falls back to the streaming reader
	bool pipeline = true;                 // LQCOV_PIPELINE=0: run_files builds a part only after the one before is mapped
	int cnt_bits = 16;                    // LQCOV_TEST_CNT_BITS (2..16): width of the match counters.  A test hook: narrower counters bring the saturated regime (sat_replay.hpp) within reach of small inputs; the oracle has the same one (LQO_CNT_BITS)
	u32 seed_bucket = 7600;               // LQCOV_SEED_BUCKET: hits per (query, slice of targets) bucket aimed at; k_seed_decide holds a bucket of up to 8192 records in registers (tests shrink it: many slices on small inputs)
	u64 seed_chunk = 1ULL << 30;          // LQCOV_SEED_CHUNK: records (8 B) of the bucket buffer; the queries of a part are bucketed in chunks of that many hits
	u32 seed_segl = 256;                  // LQCOV_SEED_SEGL: minimizers per segment (one block of the count / scatter kernels), at most LQ_SD_SEGL (tests shrink it)
	u32 seed_pair_bits = 13;              // LQCOV_SEED_PAIR_BITS: pair counters of k_seed_decide in use (tests shrink it: pairs alias on small inputs)
	u32 seed_dcap = 8192, seed_bigcap = 65536;   // LQCOV_SEED_DCAP / LQCOV_SEED_BIGCAP: records of a bucket k_seed_decide takes from registers / in passes over stretches of its targets (tests shrink them)
	u64 seed_surv_max = 2ULL << 30;       // LQCOV_SEED_SURV_MAX: survivors (8 B each) a part's plan may hold; beyond that the part is mapped without the filter (tests shrink it)
	u32 seed_hwords = 12288;              // LQCOV_SEED_HWORDS: histogram space of a bucket in words of eight bins (tests shrink it: pairs that find no room are kept as they are)
	void read_env();
};

struct SatSink {                          // where the chain kernels record a replayed query's chains (CovState::rec)
	SatRec *rec; unsigned long long *n_rec; u64 rec_cap;
	u32 *at; unsigned long long *n_at; u64 at_cap;
};

struct ReadSetDev {                       // a read set 2-bit packed in HBM, chunk aligned
	u32 n = 0;
	u64 n_chunks = 0, n_bases = 0;
	std::vector<u64> h_coff{0};           // chunk offset of every read (+ total)
	std::vector<u32> h_len;
	std::vector<std::string> names;
	DBuf codes, amb;                      // 4 x u64 / 4 x u32 per chunk
	u64 cap_chunks = 0;
	DBuf d_coff, d_len;                   // device copies of h_coff / h_len
	DBuf mx, my, moff;                    // minimizers (x, y) in emission order + per-read offsets
	u64 n_mini = 0;
	bool sketched = false;
	u64 key_stamp = 0;                    // not 0: the handle's ix_key held this set's sort keys when ix_key_stamp had the same value
	u32 dp_n = 0; u64 dp_tiles = 0;       // add_reads_packed has already run k_sketch_dp_mask over the tiles of these reads (slice by slice, under the upload of the next slice)
	u64 dp_gen = 0;                       // ... into the handle's mask buffers of that generation (lqcov_handle::sk_gen): another read set sketched since, and dp_n is void
};

// What the mapping of a part needs before its first batch, and what depends only on the part, the query set and mid_occ (not
// on what earlier parts accumulated): the probe of every query minimizer, which minimizers can repeat an x, the surviving
// seed hits (k_seed_count) and every offset that follows.  Made right after the part's index on the build stream -- under the
// mapping of the part before -- and swapped into the handle's work buffers of the same names when the part is mapped.
struct lqcov_handle;
struct SeedPlan {
	DBuf hit_start, hit_n, a_cnt, keep, dup, qdirty, dup_table, a_off, mp_off, aq_off, mpq_off, avg_qspan, qklib, mini_pos, qzero;
	DBuf surv, aqf_off;                   // the seed hits that can be part of a chain (kernels_seed.hpp), dense, as records; where every query's start
	std::vector<u64> h_aq, h_qmoff, h_aqf;
	u64 nA_total = 0, n_mp_total = 0, n_written = 0;
	i32 mid_occ = -2; u32 n_q = 0; u64 n_qm = 0;
	u32 rec_jb = 0, rec_db = 0, rec_nmin = 0;   // the records' bit layout (SeedBits); the filter's n_min
	u32 q_begin = 0, q_end = 0;           // the queries whose survivors the plan holds right now (a group of chunks; all of them unless survivors abound)
	bool bucketed = false;                // false: the first pass writes every hit (no filter asked for, or the records do not fit 64 bits): h_aqf == h_aq
	bool valid = false;
};

// One run of the seed filter (lqcov_handle::seed_filter) over the queries [q_begin, q_stop) of a part: where the part's probe
// results live right now (in the plan, or swapped into the handle while the part is mapped), where the survivors go.  A run
// ends at q_stop or when `surv` holds LQCOV_SEED_SURV_MAX survivors, whichever comes first (q_end).  Survivors are numbered
// from `base` on (aqf_off / h_aqf hold those numbers): surv[0] is survivor `base`.
struct SeedJob {
	const u64 *hit_start = nullptr; const u32 *hit_n = nullptr, *keep = nullptr; u64 *aqf_off = nullptr;
	const std::vector<u64> *h_qmoff = nullptr; std::vector<u64> *h_aqf = nullptr;
	DBuf *surv = nullptr; u64 base = 0, room_hint = 0;
	u32 q_begin = 0, q_stop = 0;
	u32 q_end = 0; u64 n_surv = 0;        // out
};

// work space of the seed filter: one plan is made at a time
struct SeedWork {
	DBuf hlen, h_off, hq_off, qg, segs, bq, cnt, off, scnt, soff, rec, has, bd, big;
	void release_large() { for (DBuf *b : { &rec, &cnt, &off, &bd }) b->release(); }   // the buffers that go by the hits of a chunk (rec: up to 8 GB): handed back when the filter ran out of memory
};

struct Part {
	bool live = false, built = false;
	SeedPlan plan;
	ReadSetDev rs;
	DBuf pos;                             // y of every minimizer, grouped by hash, ascending (index.c:188)
	DBuf tkey, tstart, tcnt;              // open-addressed table
	u32 cap_bits = 0;
	u64 n_keys = 0;
	DBuf self_off, self_rid;              // per query: same-name targets (lqmap.c:180-186)
	DBuf t_rank, q_lo;                    // -X only: name ranks for strcmp(qname, tname) > 0 (lqmap.c:187)
	AvaView ava(const lqcov_params &p) const;   // ... as the kernels take them: both null without -X (engine.cpp)
	u32 max_len() const { u32 m = 0; for (u32 v : rs.h_len) m = std::max(m, v); return m; }   // the longest target
	// the object is used again for other reads: reads, sketch and index are forgotten, the buffers stay (lqcov_part_clear; run_files' two parts)
	void clear()
	{
		rs.n = 0; rs.n_chunks = 0; rs.n_bases = 0; rs.n_mini = 0; rs.sketched = false; rs.dp_n = 0; rs.dp_tiles = 0;
		rs.h_coff.assign(1, 0); rs.h_len.clear(); rs.names.clear();
		built = false; n_keys = 0;
	}
};

// One mapping lane: a stream with its own scan/sort scratch and per-batch work space.  Query batches of a part are
// independent (lqmap.c:170-330 runs one query at a time), so lanes run them concurrently.
struct PsWork {                           // one set of psort lists + the scratch of its partition passes (kernels_psort.hpp)
	DBuf big[2], fin_s, fin_b, plan, gcnt, gcur, gdiff, tmap;
};

// What the anchor sort needs to know of a part: how many targets it holds and how long the longest one is (the key bits that vary,
// the levels that are identity passes: sort_batch).  From the part's reads (lqcov_handle::sort_geom) or stated by a test
// (lqcov_debug_sort_anchors).
// Everything the sort derives from the two numbers is derived here: the key is x = strand:1 | rid:31 | position:32 (lqmap.c:190-196),
// a level is one key byte, level 7 (shift 56) the top one.
struct SortGeom {
	u32 n_targets = 0, max_len = 0;
	constexpr u32 top_rid() const { return n_targets ? n_targets - 1 : 0; }
	constexpr u32 top_pos() const { return max_len ? max_len - 1 : 0; }
	// varying low bits of the position and of rid in this part (KeyMap)
	constexpr u32 pbits() const { u32 b = 1; while (b < 32 && ((u64)1 << b) < (u64)max_len) ++b; return b; }
	constexpr u32 rbits() const { u32 b = 0; while (b < 31 && ((u64)1 << b) < (u64)n_targets) ++b; return b; }
	KeyMap key_map() const;               // {pbits(), rbits()} (engine.cpp: KeyMap is kernels_psort.hpp's)
	// key bytes that are zero in every anchor of this part, bit i for the byte at shift 8 i: the levels sort_batch steps over.  Never the
	// strand's byte (7), the lowest byte of rid (4: shift 32 is walked even with one target) or of the position (0)
	constexpr u32 const_levels() const
	{
		return (n_targets <= (1u << 16) ? 1u << 6 : 0) | (n_targets <= (1u << 8) ? 1u << 5 : 0)
		     | (max_len <= (1u << 24) ? 1u << 3 : 0) | (max_len <= (1u << 16) ? 1u << 2 : 0) | (max_len <= (1u << 8) ? 1u << 1 : 0);
	}
	// the largest digit the byte at `shift` can hold where that is known to be less than a byte's 255: the top byte of rid or of the
	// position that varies, not the bytes below it
	constexpr u32 max_digit(u32 shift) const
	{
		return shift == 48 ? top_rid() >> 16 : shift == 40 && n_targets <= (1u << 16) ? top_rid() >> 8 : shift == 32 && n_targets <= (1u << 8) ? top_rid()
		     : shift == 24 ? top_pos() >> 24 : shift == 16 && max_len <= (1u << 24) ? top_pos() >> 16 : shift == 8 && max_len <= (1u << 16) ? top_pos() >> 8 : 255;
	}
	// buckets a pass over that byte can fill (byte 7 is strand << 7 | rid >> 24: two buckets below 2^24 targets)
	constexpr u32 max_buckets(u32 shift) const { return shift == 56 ? 2 * ((top_rid() >> 24) + 1) : max_digit(shift) + 1; }
};
namespace sort_geom_pins {                    // the values above at the edges where a bit or a level changes
constexpr u32 edges[] = {0, 1, 256, 257, 65536, 65537, 1u << 24, (1u << 24) + 1, 0x7fffffffu};
constexpr bool rid_side(u32 n, u32 rbits, u32 levels, u32 d48, u32 d40, u32 d32, u32 b56)
{
	const SortGeom g{n, 0};
	return g.rbits() == rbits && (g.const_levels() & 0xf0) == levels && g.max_digit(48) == d48 && g.max_digit(40) == d40 && g.max_digit(32) == d32 && g.max_buckets(56) == b56;
}
constexpr bool pos_side(u32 len, u32 pbits, u32 levels, u32 d24, u32 d16, u32 d8)
{
	const SortGeom g{0, len};
	return g.pbits() == pbits && (g.const_levels() & 0x0f) == levels && g.max_digit(24) == d24 && g.max_digit(16) == d16 && g.max_digit(8) == d8;
}
// every pair of edges: bytes 0, 4 and 7 are never stepped over, a level that is stepped over holds one digit, and the bytes without a
// bound (7 and 0 always) say 255
constexpr bool consistent()
{
	for (u32 n : edges) for (u32 len : edges) {
		const SortGeom g{n, len};
		if (g.const_levels() & 0x91) return false;
		for (u32 lv = 0; lv < 8; ++lv) {
			if ((g.const_levels() >> lv & 1) && g.max_digit(8 * lv) != 0) return false;
			if (lv != 7 && g.max_buckets(8 * lv) != g.max_digit(8 * lv) + 1) return false;
		}
		if (g.max_digit(56) != 255 || g.max_digit(0) != 255) return false;
	}
	return true;
}
static_assert(consistent(), "SortGeom: a constant level with more than one digit, or a level that must be walked marked constant");
//                     targets      rbits levels  >>16   >>8  byte 4  buckets at 56
static_assert(rid_side(0,             0,  0x60,     0,     0,     0,    2), "");
static_assert(rid_side(1,             0,  0x60,     0,     0,     0,    2), "");
static_assert(rid_side(256,           8,  0x60,     0,     0,   255,    2), "");
static_assert(rid_side(257,           9,  0x40,     0,     1,   255,    2), "");
static_assert(rid_side(65536,        16,  0x40,     0,   255,   255,    2), "");
static_assert(rid_side(65537,        17,  0x00,     1,   255,   255,    2), "");
static_assert(rid_side(1u << 24,     24,  0x00,   255,   255,   255,    2), "");
static_assert(rid_side((1u << 24) + 1, 25, 0x00,  256,   255,   255,    4), "");   // (rid >> 16 is not cut to a byte: 256 and up mean "any digit")
static_assert(rid_side(0x7fffffffu,  31,  0x00, 32767,   255,   255,  256), "");
//                     longest      pbits levels  >>24  >>16   >>8
static_assert(pos_side(0,             1,  0x0e,     0,     0,     0), "");
static_assert(pos_side(1,             1,  0x0e,     0,     0,     0), "");
static_assert(pos_side(256,           8,  0x0e,     0,     0,     0), "");
static_assert(pos_side(257,           9,  0x0c,     0,     0,     1), "");
static_assert(pos_side(65536,        16,  0x0c,     0,     0,   255), "");
static_assert(pos_side(65537,        17,  0x08,     0,     1,   255), "");
static_assert(pos_side(1u << 24,     24,  0x08,     0,   255,   255), "");
static_assert(pos_side((1u << 24) + 1, 25, 0x00,    1,   255,   255), "");
static_assert(pos_side(0x7fffffffu,  31,  0x00,   127,   255,   255), "");
}

// One call of sort_checked as lqcov_set_debug's bit 1 records it (lqcov_get_sort_batches)
struct SortBatchRec {
	u32 kind = 0;                         // 0: every hit, klib's order (LQCOV_TIES=klib; the replay of a saturated query), 1: first pass, 2: second pass
	std::vector<u32> q, klib;             // the engine's query numbers; which of them went through klib's passes
	std::vector<u64> off;                 // per-query anchor offsets (q.size() + 1)
	std::vector<mm128> emitted, sorted;
};

struct MapLane {
	int id = 0;                           // its place in lqcov_handle::lanes (add_lane): the timeline's lane number
	hipStream_t stream = nullptr;         // klib's passes (queries with repeated minimizers), then runs and chains
	hipStream_t stream2 = nullptr;        // the parallel sort of every other query, meanwhile
	hipStream_t streamW = nullptr;        // the serial token walks: streams confined to a quarter of the CUs (see map_part):
	hipStream_t streamW2 = nullptr;       //   checkpointed walks + their solvers | whole walks of the shorter size classes
	hipEvent_t ev_fork = nullptr, ev_join = nullptr, ev_w0 = nullptr, ev_w1 = nullptr, ev_w2 = nullptr;
	DBuf sort_cnt, mhist;
	DBuf ck_segs, ck_T, ck_E, ck_S, ck_slot, ck_n;   // checkpointed walks (kernels_ckpt.hpp)
	PsWork ps[2];
	Prim prim;
	bool gate_passed = false;             // this batch has reached its long walks (see map_part)
	bool prune = false; u32 prune_n_want = 0, prune_n_sub = 0;   // second pass: klib's levels drop the buckets without a listed run (k_rs_children; L.want, L.sub_off, L.sub_q)
	DBuf sens, n_sens, want, sub_q, sub_off, sub_klib;   // runs left to the second pass (map_batch), its queries
	DBuf A, B, R0, segs0, segs1, n_segs, hist, begs;     // A: anchors (final home), B: originals of the klib queries / other buffer of the parallel sort, R0: records (R1 lives in scr)
	DBuf tile_list, two_tiles, two_tile0, two_tcnt, two_m;
	DBuf sort_d, sort_dst, seg_info, walk_list, two_list, scr;
	DBuf gsel, gkey, gsel2, gkey2, gstart, run_tiles, sel_tiles;
	DBuf ivl, n_ivl, iv_q, iv_q2, iv_se, iv_se2, ivq_off, iv_scratch;
	DBuf arena_buf; LqArena arena;        // the lane's work space (prim.hpp): its buffers are pieces of it, for the length of a batch
	// every buffer of the lane, for the two functions below
	template <class F> void each_buffer(F f)
	{
		for (DBuf *b : { &sens, &n_sens, &want, &sub_q, &sub_off, &sub_klib, &sort_cnt, &mhist, &ck_segs, &ck_T, &ck_E, &ck_S, &ck_slot, &ck_n, &prim.tmp, &A, &B, &R0, &segs0, &segs1, &n_segs, &hist, &begs, &tile_list, &two_tiles, &two_tile0, &two_tcnt, &two_m,
		                 &sort_d, &sort_dst, &seg_info, &walk_list, &two_list, &scr, &gsel, &gkey, &gsel2, &gkey2, &gstart, &run_tiles, &sel_tiles,
		                 &ivl, &n_ivl, &iv_q, &iv_q2, &iv_se, &iv_se2, &ivq_off, &iv_scratch }) f(*b);
		for (PsWork &W : ps) for (DBuf *b : { &W.big[0], &W.big[1], &W.fin_s, &W.fin_b, &W.plan, &W.gcnt, &W.gcur, &W.gdiff, &W.tmap }) f(*b);
	}
	// hand every buffer back (they regrow on the next batch); the caller has drained the lane's streams
	void release_buffers() { each_buffer([](DBuf &b) { b.release(); }); arena.used = 0; arena.base = nullptr; arena.size = 0; arena_buf.release(); }
	// a new batch starts with an empty arena: the pieces the last batch cut from it are forgotten
	void drop_arena_buffers() { each_buffer([](DBuf &b) { if (b.in_arena) b.release(); }); arena.used = 0; }
};

struct lqcov_handle {
	lqcov_params P;
	Knobs K;
	MapParams mp;
	int device = 0;
	hipStream_t stream = nullptr;         // queries, the head of map_part, finish
	hipStream_t bstream = nullptr;        // upload, sketch and index of a part (with bprim): another part may be mapped meanwhile
	hipStream_t cstream = nullptr;        // the upload of packed reads in slices: a slice is sketched on bstream while the next one arrives
	hipEvent_t ev_up[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
	Prim prim, bprim;
	u64 hbm_reserve = 0;                  // bytes the caller wants left free when the lanes size their work space (a second part being built)
	std::string err;
	int profiling = 0;                    // 0 off, 1 per-kernel (waits for every kernel, lanes run in turn), 2 events only (read when asked)
	std::string profile_only;             // if not empty: only this stage is timed
	struct StagePending { const char *name; hipEvent_t a, b; u64 bytes; };
	std::vector<StagePending> stage_pending; std::mutex stage_mu;
	void account_stage(const char *name, hipEvent_t a, hipEvent_t b, u64 bytes);
	void add_stage_bytes(const char *name, u64 bytes);       // algorithmic bytes known only after the fact (device-side tallies)
	std::map<std::string, u64> late_bytes;
	void drain_stages();
	u32 debug_flags = 0;                  // lqcov_set_debug: bit 0 records chains, bit 1 what every sort was handed and what it made of it
	std::vector<SortBatchRec> sort_recs; std::mutex sort_rec_mu;   // bit 1: the sorts of the last map_part
	bool distributed = false;             // per-part accumulators, COVT replayed by the caller (multi-GPU)
	std::map<std::string, StageAcc> stages;
	std::vector<std::string> stage_order;

	// query set and per-query accumulators
	ReadSetDev q;
	bool have_queries = false, q_has_qual = false;
	// queries are held longest first (anchors per query grow with its length: the batch with the longest serial walks then
	// starts first and the last batch has the shortest); q_perm[internal] = position in the caller's order, q_inv the inverse.
	// Everything per query inside the engine (and in the accumulator exchange of the multi-GPU path) uses the internal order;
	// rows, regions, minimizer and chain dumps are handed out in the caller's order.
	std::vector<u32> q_perm, q_inv;
	// Query sets (lqcov_set_query_sets): set s holds the caller's queries set_first[s] .. set_first[s + 1] - 1, mapped with its own
	// -p / -q; q_thr holds med << 16 | good per query in the internal order (CovState::thr).  One set, no q_thr: lqcov_set_queries.
	std::vector<u32> set_first;
	DBuf q_thr; bool have_thr = false;
	DBuf q_owner;                         // query of every query minimizer
	DBuf lambda, lambda2, avg_k, cnts, qflags, qual_psum;
	DBuf dup, qdirty, dup_table;          // k_dup_mark: minimizers / queries whose anchors can repeat an x (per part)
	DBuf qklib;                           // queries that go through klib's passes (per part): marked and more than 64 anchors
	DBuf qzero;                           // zeros: nobody goes through klib's passes (first pass of map_batch)
	DBuf surv, aqf_off;                   // the part's surviving seed hits as records and their per-query offsets (SeedPlan, swapped in by map_part)
	SeedWork seed_ws; std::mutex seed_mu;  // work space of the seed filter: one plan (or group of a plan) is made at a time, whichever thread asks
	// Queries one of whose match counters reached cnt_max (uint16 in the reference: 65535; esterr.c:130,136): from the part in
	// which that happens on, their counters live here, replayed part by part in the reference's chain order (sat_replay.hpp,
	// sat_replay_part), and go back to the device before the rows are made.  Key: the query in the engine's order.
	std::map<u32, std::vector<u32>> sat_cnt;
	u32 cnt_max = 65535;                  // (LQCOV_TEST_CNT_BITS)
	DBuf sat_rec, sat_at, sat_n;
	u64 stat_sat_chains = 0;
	std::vector<SatRec> sat_last_recs; std::vector<u32> sat_last_at;   // lqcov_part_sat_records: the records between the sizing call and the copying one
	int sat_last_part = -1; u32 sat_last_query = 0;
	std::atomic<bool> sat_last_valid{false};   // ... which describe the part as it was: dropped by reset() and whenever a part is cleared, released, built or mapped (the build thread may be the one)
	u64 last_n_written = 0;               // anchors the first pass wrote against the last part
	std::atomic<u64> stat_tie_why[6] = {};   // listed runs by the first reason that listed them (lq_tie_list: skip pending, member counts as a skip, top score twice, scan broke off, peak tie, other), since reset()
	std::atomic<u64> stat_sens_runs{0}, stat_p2_queries{0}, stat_p2_anchors{0};   // second pass, since reset(): runs, queries, anchors
	u32 run_n_min() const { const i32 span_max = P.hpc ? 255 : P.k; return (u32)std::max<i32>(std::max<i32>(P.min_cnt, 1), (mp.min_sc + span_max - 1) / span_max); }   // anchors a run needs to hold a chain (k_run_list)
	// counter layout: normally the query minimizer offsets; after adopt_index_params() (prebuilt index with other -k/-w/-H)
	// the reference's sizes (from the command-line sketch, minimap2-coverage.c:419-422) and the mapping's differ
	bool own_cnt_layout = false; DBuf cnt_off, d_nsize; std::vector<u32> h_nsize; u64 cnt_total = 0;
	const u64 *cnt_off_dev() const { return own_cnt_layout ? cnt_off.as<u64>() : q.moff.as<u64>(); }
	u64 cnt_count() const { return own_cnt_layout ? cnt_total : q.n_mini; }
	DBuf pv; DBuf n_pv; u32 pv_cap = 0;   // persisted intervals + markers (ovlp_coords)
	i32 mid_occ = -1;

	std::vector<std::unique_ptr<Part>> parts;

	// work buffers of part_map
	DBuf hit_start, hit_n, a_cnt, keep, a_off, mp_off, mini_pos, aq_off, mpq_off, avg_qspan, skip;
	std::vector<std::unique_ptr<MapLane>> lanes;
	int n_lanes = 3;
	std::mutex pv_mu; u64 pv_reserved = 0;
	std::mutex gate_mu; std::condition_variable gate_cv; int gate_count = 0;   // staggered lane start
	DBuf dbg_chains, n_dbg; u64 dbg_cap = 0; u64 n_dbg_host = 0;
	DBuf misc;
	DBuf ix_key, ix_key2, ix_head, ix_uidx, ix_ukey, ix_ustart, ix_ucnt, ix_sorted;   // build_index workspaces
	const Part *ix_owner = nullptr;       // the part ix_ukey / ix_ustart / ix_ucnt describe (dump_part reads them)
	u64 ix_key_stamp = 0, ix_key_seq = 0; // ix_key holds the sort keys of the read set with this stamp (written by k_sketch_emit_mask with its x and y)
	DBuf sk_ulist;                        // sketch: the chunks the data-parallel kernel left to the machine + their count
	DBuf sk_cnt, sk_off, sk_owned, sk_mask, sk_flag, sk_toff, sk_trid, sk_grid;   // sketch: per-chunk minimizer counts / offsets, which kernel decides a chunk, emitted positions (a bit per base), tile offsets
	std::vector<u64> sk_h_toff;           // tiles of k_sketch_dp_mask before every read (host copy of sk_toff)
	const ReadSetDev *sk_owner = nullptr; u64 sk_gen = 0;   // whose reads the sk_* buffers describe right now (sketch_dp_setup): a read set's dp_n counts only while they are its own
	u64 last_n_anchors = 0;
	u64 anchor_budget = 0;

	// finish()
	bool finished = false;
	std::vector<lqcov_row> rows;
	std::vector<lqcov_region> regs, mregs;

	lqcov_handle(const lqcov_params &p, int dev);
	~lqcov_handle();

	void add_reads(ReadSetDev &rs, u32 n, const u8 *seq, const u64 *seq_off, const char *names, const u64 *name_off);
	void amb_tails(ReadSetDev &rs, u32 r0, u32 r1, u64 chunk0, u64 n_chunks);
	void add_reads_packed(ReadSetDev &rs, u32 n, const u64 *codes, const u32 *amb, const u32 *lens, const char *names, const u64 *name_off,
	                      const u64 *codes_dev = nullptr, const u32 *amb_dev = nullptr, u64 stride_chunks = 0, const std::vector<u64> *share_chunks = nullptr);
	void sketch(ReadSetDev &rs, bool rid_in_y);
	bool sketch_dp_setup(ReadSetDev &rs, u64 &n_tiles);
	void sketch_dp_launch(ReadSetDev &rs, u64 tile0, u64 tile1);
	void export_minimizers(ReadSetDev &rs, u64 *x_dev, u64 *y_dev, u32 rid_base);
	void set_queries(u32 n, const u8 *seq, const u64 *seq_off, const u8 *qual, const char *names, const u64 *name_off, bool batch_rule = true);
	void set_query_sets(u32 n, const u8 *seq, const u64 *seq_off, const u8 *qual, const char *names, const u64 *name_off,
	                    u32 n_sets, const u32 *first, const i32 *med, const i32 *good);
	void build_index(Part &pt);
	void build_part(Part &pt);
	void open_gate();
	void plan_part(Part &pt, hipStream_t s, Prim &pr);
	// plan_part's steps
	void pp_probe_marks(Part &pt, hipStream_t s);
	void pp_survivors(Part &pt, hipStream_t s, Prim &pr);
	bool seed_group_or_not(Part &pt, SeedPlan &S, bool swapped, hipStream_t s, Prim &pr, u32 q_begin);   // seed_group; false also where it ran out of memory
	void rest_unfiltered(SeedPlan &S, DBuf &aqf, const DBuf &aq, u32 from, hipStream_t s);                // the queries from `from` on without the filter
	bool plan_usable(const SeedPlan &S) const;   // the plan was made for these queries, this mid_occ and tie order, and holds its first group of survivors: the part can be mapped from it
	bool seed_filter(Part &pt, hipStream_t s, Prim &pr, SeedWork &W, u32 n_min, u32 jb, u32 db, SeedJob &J);
	bool seed_group(Part &pt, SeedPlan &S, bool swapped, hipStream_t s, Prim &pr, u32 q_begin);
	// seed_filter's steps
	std::vector<u64> sf_query_hits(hipStream_t s, Prim &pr, SeedWork &W, const SeedJob &J);
	SeedRun sf_inputs(Part &pt, SeedWork &W, const SeedJob &J, u32 n_min, u32 jb, u32 db);
	u32 sf_chunk(hipStream_t s, Prim &pr, SeedWork &W, SeedRun &R, const SeedChunk &c);
	void swap_plan(SeedPlan &S);
	u64 part_seed_survivors(Part &pt, u32 info[4], u64 *off, u64 off_cap, u32 *rows, u64 row_cap);   // tests: the plan's survivors, decoded (lqcov_part_seed_survivors)
	void map_part(Part &pt);
	// map_part's steps
	void mp_prologue(Part &pt, bool dbg);
	void mp_arenas(Part &pt);
	void mp_pv_room(u64 nA_total);
	void run_batches(Part &pt, const std::vector<std::pair<u32, u32>> &batches, bool dbg);
	void grow_pv(u32 npv, u64 want_bytes, hipStream_t s);
	void map_batch(MapLane &L, Part &pt, u32 q0, u32 q1, const std::vector<u64> &h_aq, const std::vector<u64> &h_aqf, const std::vector<u64> &h_qmoff, bool dbg);
	// map_batch's steps
	void mb_emit(MapLane &L, Part &pt, u32 q0, u32 q1, const std::vector<u64> &h_qmoff, u64 a_base, u64 nA);
	void mb_first_pass(MapLane &L, Part &pt, u32 q0, u32 q1, const std::vector<u64> &h_off, u64 a_base, u64 nA, u32 ivl_cap, bool dbg);
	void mb_second_pass(MapLane &L, Part &pt, u32 n_sens, const std::vector<u64> &h_aq, const std::vector<u64> &h_qmoff, u32 ivl_cap, bool dbg);
	void emit_hits(MapLane &L, Part &pt, dim3 grid, u64 j0, u64 nj, u64 a_base, const u32 *klib, const EmitSub &sub, u64 bytes);
	void batch_buffers(MapLane &L, u64 nA);
	void chain_stage(MapLane &L, Part &pt, const u64 *aqb, u64 a_base, u32 nqb, u32 q0, const u32 *qmap, u64 nA, int tie_mode, u32 n_want, u32 ivl_cap, bool dbg, const SatSink *sink = nullptr);
	void map_subset(MapLane &L, Part &pt, const std::vector<u32> &sq, const std::vector<u32> &sk, const std::vector<u64> &so, u64 max_mini, int tie_mode, u32 n_want, u32 ivl_cap, bool dbg, const SatSink *sink);
	void debug_sort_pairs(u64 *keys, u64 *vals, u64 n, unsigned bits, int key_bytes);   // tests: the primitives of kernels_isort.hpp on host arrays
	void debug_scan(const u32 *in, u64 *out, u64 n);
	void debug_sort_anchors(u64 *xy, u64 n, const u64 *q_off, const u32 *q_klib, u32 n_q, SortGeom g, const u64 *want, u32 n_want);   // tests: sort_batch on anchors from the host
	bool filter_intervals(MapLane &L, u32 ni);                  // the per-part filter on the ni intervals of L.ivl (map_batch); true: pv grew
	void debug_filter_intervals(const u32 *iv, u32 n, u32 info[2]);   // tests: filter_intervals on intervals from the host
	void add_lane();
	static SortGeom sort_geom(const Part &pt);
	bool sat_chains(Part &pt, u32 qi, const std::vector<u64> &h_aq, const std::vector<u64> &h_qmoff, std::vector<SatRec> &recs, std::vector<u32> &at);
	void sat_check(const std::vector<SatRec> &recs, const std::vector<u32> &at, size_t nc);
	void part_sat_records(Part &pt, u32 qi, std::vector<SatRec> &recs, std::vector<u32> &at);
	void sat_replay_host(u32 qi, const SatRec *recs, u64 n_recs, const u32 *at, u64 n_at, u32 *counters, u64 n_counters);
	void sat_replay_part(Part &pt, const std::vector<u64> &h_aq, const std::vector<u64> &h_qmoff);
	void sort_checked(MapLane &L, SortGeom g, const u64 *aqb, const u32 *qkb, u32 nqb, u64 a_base, u64 nA, const std::vector<u64> &h_off, const std::vector<u32> &h_klib, u32 kind, const u32 *h_q);
	void sort_batch(MapLane &L, SortGeom g, const u64 *aqb, const u32 *qkb, u32 nqb, u64 a_base, u64 nA);
	void psort_run(MapLane &L, int set, hipStream_t s, u64 nA, const KeyMap &km, const struct PsData &pd);
	void psort_tail(MapLane &L, int set, hipStream_t s, u64 nA, const KeyMap &km, const struct PsData &pd);
	void reset();
	void finish();
	void write_table(FILE *out);
	void write_table_set(u32 set, FILE *out);
	struct QuerySetFiles { std::vector<const char *> paths; std::vector<i32> med, good; std::vector<FILE *> outs; };
	// the whole run from files, and the table as text above: runfiles.cpp.  sets != null: the queries are the files of `sets` (query and
	// out are not used), one table per set
	int run_files(const char *target, const char *query, FILE *out, FILE *log, const char *dump_path = nullptr, const QuerySetFiles *sets = nullptr);
	void adopt_index_params(i32 k, i32 w, i32 hpc);
	void dump_part(Part &pt, FILE *fp);                      // mm_idx_dump (index.c:390-426)
	bool load_part(FILE *fp, Part &pt);                      // mm_idx_load (index.c:428-479); false at end of file
	void build_part_from_host_minimizers(Part &pt, const std::vector<u64> &x, const std::vector<u64> &y,
	                                     std::vector<std::string> &&names, std::vector<u32> &&lens);
	Part &part(int id);
};

// a part's plan stands in the handle's work buffers (swap_plan) for as long as this lives
struct PlanGuard { lqcov_handle *h; SeedPlan &S; ~PlanGuard() { h->swap_plan(S); } };

u64 lq_packed_chunks(u32 n, const u64 *seq_off);
#include <functional>
// The reference's rule for cutting n target reads into index parts, from their lengths alone (index.c:244,311-316 and bseq.c:86-98):
// reads are taken in mini-batches, each ending with the read that brings it to min(idx_mini_batch, -I) bases, and a part takes
// mini-batches while its running total is <= -I.  -> [first, last) read of every part.
template <class LenAt>
std::vector<std::pair<size_t, size_t>> lq_part_ranges(size_t n, LenAt len_at, u64 batch_size, u64 idx_mini_batch)
{
	const i64 chunk = (int)(idx_mini_batch < batch_size ? idx_mini_batch : batch_size);   // index.c:316
	std::vector<std::pair<size_t, size_t>> ranges;
	size_t r0 = 0;
	while (r0 < n) {
		u64 sum_len = 0; size_t r1 = r0;
		while (r1 < n && sum_len <= batch_size) {
			i64 size = 0;
			while (r1 < n) { size += (i64)len_at(r1); ++r1; if (size >= chunk) break; }
			sum_len += (u64)size;
		}
		ranges.emplace_back(r0, r1);
		r0 = r1;
	}
	return ranges;
}
void lq_format_rows(FILE *out, int filter_flag, const lqcov_row *rows, u32 n_rows, const lqcov_region *regs, const lqcov_region *mregs,
                    const std::function<const char *(u32)> &name_of);
void lq_pack_host(u32 n, const u8 *seq, const u64 *seq_off, u64 *codes, u32 *amb, int n_threads);
bool lq_packed_read_ambiguous(const u32 *aw, u64 len);
void lq_make_q2p(double *t);                              // meanQ's table of 127 error probabilities (lqutils.c:26-49)

struct StageTimer {
	lqcov_handle *h; hipStream_t s; const char *name; u64 bytes;
	hipEvent_t a = nullptr, b = nullptr; bool on = false;
	StageTimer(lqcov_handle *h_, const char *name_, u64 bytes_ = 0);
	StageTimer(lqcov_handle *h_, hipStream_t s_, const char *name_, u64 bytes_ = 0);
	~StageTimer();
};
