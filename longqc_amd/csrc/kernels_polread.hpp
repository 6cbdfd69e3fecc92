// longqc_amd/csrc/kernels_polread.hpp -- the polymerase reads of a Sequel run from its two unaligned BAMs: what lq_sequel.run_platformqc
// (lq_sequel.py:25-137, 260-336; get_N50 / get_NXX of lq_utils.py:33-53) computes between opening *.scraps.bam / *.subreads.bam and
// its JSON block.  Nothing of a record is used but its name "movie/zmw/start_end" and, in the scraps file, the two one-byte tags sz
// and sc.  The host side is polread.cpp, the caller longqc_amd/sequel.py; DESIGN 8 (20) has the domain and the order.
//
//   k_pol_fields   one lane per row of the device record walk (kernels_bamscan.hpp): the name parsed into zmw, start, end; in the scraps
//                  file the aux area walked from behind the qualities to the record's end for the first sz and the first sc, every value
//                  type of the SAM specification's 4.2.4 skipped by its size (B by subtype and count, Z and H to their NUL), never a byte
//                  read at or behind the record's end.  tmp[r] = the record's item, flags[r] = LQ_POL_ITEM / LQ_POL_FLAGGED / LQ_POL_CONTROL,
//                  cols[t] = the tile's slots.  A record outside the domain is FLAGGED and keeps a slot: the host twin (polread.cpp) re-reads
//                  it and fills the slot in, so the items stay in record order.  The control throughput (sz C, sc F: end - start + 1) and
//                  the number of flagged records: a block reduction and one atomic each per block.
//   k_pol_compact  (after k_fx_tilescan over cols) items[first + slot] = tmp[r]: the items of a piece behind those of the pieces before.
//   k_pol_keys     the two sort keys of every item: end, and zmw << 32 | start; value = the item's index, which is its arrival index
//                  (scraps before subreads, each in file order).  Two stable passes of the engine's radix sort (kernels_isort.hpp), by end and
//                  then by (zmw, start), give the total order (zmw, start, end, arrival): sorted(key=itemgetter(0, 1)) per ZMW, ties included.
//                  An empty slot (a flagged record that yields nothing) has zmw LQ_POL_VOID and sorts behind every item.
//   k_pol_order    sorted[i] = items[idx[i]], flag[i] = 1 where zmw changes (flag[n] = 0 for the scan of n + 1 entries).
//   k_pol_heads    head[pos[i]] = i where flag[i], head[groups] = n.
//   k_pol_walk     construct_polread's pass over one ZMW's items, one lane per ZMW, int64 throughout.  A ZMW of more than LQ_POL_LONG_ITEMS
//                  items is put on a list and walked, again one lane each, by a second launch over that list: beside lanes of tens of items
//                  it would hold its wave for thousands of steps.  (The pass is not written as a scan: DESIGN 8 (20) says why.)
//   k_pol_pack     the is_pol ZMWs' hq and tot as uint32 arrays in zmw order (pos: the scan of the is_pol flags), their adapter counts, the
//                  descending sort key ~hq, and the run's sums: sum hq, max hq, min / max tot, min / max ad_num, flagged ZMWs.
//   k_pol_unkey    v[i] = ~k[i] after the keys-only sort: hq in descending order.
//   k_pol_nxx      from v and its exclusive scan: N50 = v[i] at the first i with 2 cum[i] >= sum, N90 at the first with 100 cum[i] >= 90 sum
//                  (cum inclusive).  Integer comparisons: equal to the reference's float ones while 100 sum < 2^53 (the host asserts it).
// Tiles and threads are the record walk's (LQ_FXSCAN_THREADS, lq_fx_block_scan, k_fx_tilescan); every kernel strides over its grid.
#pragma once
#include "kernels_fxscan.hpp"

#define LQ_POL_THREADS 256
#define LQ_POL_MAX_BLOCKS 1024u       // tiles / elements are strided over the blocks of a launch
#define LQ_POL_LONG_ITEMS 256         // a ZMW with more items than this is walked by the second launch
#define LQ_POL_MAX_DIGITS 9           // zmw, start, end: 1 .. 9 ASCII digits (below 2^30)
#define LQ_POL_VOID 0x7fffffffu       // zmw of an empty slot
#define LQ_POL_CLASS_OTHER 1u         // an item's class where sc is no single character (host twin only): it acts like every class but L, S, A
static_assert(LQ_POL_THREADS == LQ_FXSCAN_THREADS, "lq_fx_block_scan scans a block of LQ_FXSCAN_THREADS");
constexpr u32 LQ_POL_LONG = LQ_POL_LONG_ITEMS;

#define LQ_POL_ITEM    1u             // the record gives an item (tmp[r]; its slot is taken)
#define LQ_POL_FLAGGED 2u             // outside the domain: the host twin decides (its slot is taken and holds LQ_POL_VOID until then)
#define LQ_POL_CONTROL 4u             // sz C, sc F: end - start + 1 went into the control throughput

struct alignas(16) PolItem { u32 zmw, start, end, cls; };
struct PolSums { unsigned long long sum_hq, max_hq, min_tot, max_tot, n_flagged, n_range; u32 min_ad, max_ad; unsigned long long n50, n90; };

// 1 .. 9 digits at p[q .. lim) -> *val, q behind them; false: none, or a tenth
__host__ __device__ __forceinline__ bool lq_pol_digits(const u8 *p, u64 &q, u64 lim, u32 *val)
{
	u32 v = 0, n = 0;
	while (q < lim) {
		const u32 c = (u32)p[q] - '0';
		if (c > 9) break;
		if (n == LQ_POL_MAX_DIGITS) return false;
		v = v * 10 + c; ++n; ++q;
	}
	*val = v;
	return n != 0;
}

// the name p[q .. lim) = "movie/zmw/start_end": true if it lies in the domain
__host__ __device__ __forceinline__ bool lq_pol_name(const u8 *p, u64 q, u64 lim, PolItem *it)
{
	while (q < lim && p[q] != '/') ++q;
	if (q >= lim) return false;
	const u64 z0 = ++q;
	if (!lq_pol_digits(p, q, lim, &it->zmw) || q >= lim || p[q] != '/') return false;
	if (p[z0] == '0' && q - z0 > 1) return false;             // (ZMWs are keyed by their text: "007" is not "7")
	++q;
	if (!lq_pol_digits(p, q, lim, &it->start) || q >= lim || p[q] != '_') return false;
	++q;
	if (!lq_pol_digits(p, q, lim, &it->end)) return false;
	return q == lim || p[q] == '_' || p[q] == '/';
}

// bytes of a value of type ty (A c C s S i I f, and the subtypes of B), 0: none of them
__host__ __device__ __forceinline__ u32 lq_pol_scalar(u32 ty, bool with_a)
{
	switch (ty) {
	case 'A': return with_a ? 1 : 0;
	case 'c': case 'C': return 1;
	case 's': case 'S': return 2;
	case 'i': case 'I': case 'f': return 4;
	default: return 0;
	}
}

// the aux area p[a .. end): the first sz and sc (type << 8 | first value byte, 0: absent).  false: it does not end exactly at `end`
__host__ __device__ __forceinline__ bool lq_pol_aux(const u8 *p, u64 a, u64 end, u32 *sz, u32 *sc)
{
	*sz = *sc = 0;
	while (a + 3 <= end) {
		const u32 t0 = p[a], t1 = p[a + 1], ty = p[a + 2];
		const u64 v = a + 3;
		u64 len = lq_pol_scalar(ty, true);
		if (!len) {
			if (ty == 'Z' || ty == 'H') {
				u64 z = v;
				while (z < end && p[z]) ++z;
				if (z >= end) return false;
				len = z - v + 1;
			} else if (ty == 'B') {
				if (v + 5 > end) return false;
				const u64 es = lq_pol_scalar(p[v], false);
				if (!es) return false;
				len = 5 + es * ((u64)p[v + 1] | (u64)p[v + 2] << 8 | (u64)p[v + 3] << 16 | (u64)p[v + 4] << 24);
			} else return false;
		}
		if (v + len > end) return false;
		if (t0 == 's' && t1 == 'z' && !*sz) *sz = ty << 8 | p[v];
		if (t0 == 's' && t1 == 'c' && !*sc) *sc = ty << 8 | p[v];
		a = v + len;
	}
	return a == end;
}

// the record at p[rec ..) of a file of `kind` (0 scraps, 1 subreads), whole and vouched for by the record walk; name_len: up to the
// name's first NUL -> its flags; *it its item, *control what it adds to the control throughput
__host__ __device__ __forceinline__ u32 lq_pol_record(const u8 *p, u64 rec, u32 name_len, int kind, PolItem *it, i64 *control)
{
	it->zmw = LQ_POL_VOID; it->start = it->end = it->cls = 0;
	*control = 0;
	u32 cls = 'S';
	bool is_control = false;
	if (kind == 0) {
		const u64 block_size = (u64)p[rec] | (u64)p[rec + 1] << 8 | (u64)p[rec + 2] << 16 | (u64)p[rec + 3] << 24;
		const u64 l_name = p[rec + 12], n_cigar = (u64)p[rec + 16] | (u64)p[rec + 17] << 8;
		const u64 l_seq = (u64)p[rec + 20] | (u64)p[rec + 21] << 8 | (u64)p[rec + 22] << 16 | (u64)p[rec + 23] << 24;
		u32 sz, sc;
		if (!lq_pol_aux(p, rec + 36 + l_name + 4 * n_cigar + (l_seq + 1) / 2 + l_seq, rec + 4 + block_size, &sz, &sc)) return LQ_POL_FLAGGED;
		if (!sz || !sc) return 0;
		if (sz >> 8 != 'A' || sc >> 8 != 'A') return LQ_POL_FLAGGED;
		sz &= 0xff; cls = sc & 0xff;
		if (sz == 'C') is_control = true;
		else if (sz != 'N') return 0;
	}
	PolItem x;
	if (!lq_pol_name(p, rec + 36, rec + 36 + name_len, &x)) return LQ_POL_FLAGGED;
	if (is_control) {
		if (cls != 'F') return 0;
		*control = (i64)x.end - (i64)x.start + 1;
		return LQ_POL_CONTROL;
	}
	it->zmw = x.zmw; it->start = x.start; it->end = x.end; it->cls = cls;
	return LQ_POL_ITEM;
}

// rows[0 .. n_rows): the record walk's rows, positions relative to base + org.  cols[t] = the slots of tile t; ctl[0] += the control
// throughput, ctl[1] += the flagged records (the host zeroes ctl)
static __global__ void __launch_bounds__(LQ_POL_THREADS)
k_pol_fields(const u8 *base, u32 org, const FxRow *rows, u64 n_rows, int kind, PolItem *tmp, u32 *flags, u64 *cols, unsigned long long *ctl)
{
	__shared__ u64 wsum[LQ_POL_THREADS / 64];
	const u64 n_tiles = (n_rows + LQ_FXSCAN_LINE_TILE - 1) / LQ_FXSCAN_LINE_TILE;
	u64 control = 0, n_flagged = 0;
	for (u64 t = blockIdx.x; t < n_tiles; t += gridDim.x) {
		const u64 r = t * LQ_FXSCAN_LINE_TILE + threadIdx.x;
		u32 f = 0;
		if (r < n_rows) {
			const FxRow row = rows[r];
			PolItem it; i64 c;
			f = lq_pol_record(base, (u64)org + row.name_at - 36, row.name_len, kind, &it, &c);
			tmp[r] = it; flags[r] = f;
			control += (u64)c;
			n_flagged += f & LQ_POL_FLAGGED ? 1 : 0;
		}
		u64 tot;
		lq_fx_block_scan(f & (LQ_POL_ITEM | LQ_POL_FLAGGED) ? 1 : 0, wsum, &tot);
		if (threadIdx.x == 0) cols[t] = tot;
	}
	u64 tot_c, tot_f;
	lq_fx_block_scan(control, wsum, &tot_c);                     // (two's complement: a negative end - start + 1 adds as it should)
	lq_fx_block_scan(n_flagged, wsum, &tot_f);
	if (threadIdx.x == 0) {
		if (tot_c) atomicAdd(ctl, (unsigned long long)tot_c);
		if (tot_f) atomicAdd(ctl + 1, (unsigned long long)tot_f);
	}
}

// cols scanned: items[cols[t] + the record's rank among its tile's slots] = tmp[r]
static __global__ void __launch_bounds__(LQ_POL_THREADS)
k_pol_compact(const PolItem *tmp, const u32 *flags, u64 n_rows, const u64 *cols, PolItem *items)
{
	__shared__ u64 wsum[LQ_POL_THREADS / 64];
	const u64 n_tiles = (n_rows + LQ_FXSCAN_LINE_TILE - 1) / LQ_FXSCAN_LINE_TILE;
	for (u64 t = blockIdx.x; t < n_tiles; t += gridDim.x) {
		const u64 r = t * LQ_FXSCAN_LINE_TILE + threadIdx.x;
		const bool slot = r < n_rows && (flags[r] & (LQ_POL_ITEM | LQ_POL_FLAGGED));
		u64 tot;
		const u64 ex = lq_fx_block_scan(slot ? 1 : 0, wsum, &tot);
		if (slot) items[cols[t] + ex] = tmp[r];
	}
}

static __global__ void __launch_bounds__(LQ_POL_THREADS)
k_pol_keys(const PolItem *items, u64 n, u32 *k_end, u64 *idx, u64 *k_zs)
{
	for (u64 i = (u64)blockIdx.x * LQ_POL_THREADS + threadIdx.x; i < n; i += (u64)gridDim.x * LQ_POL_THREADS) {
		const PolItem it = items[i];
		k_end[i] = it.end; idx[i] = i;
		k_zs[i] = (u64)it.zmw << 32 | it.start;
	}
}

// k2[i] = k_zs[idx[i]]: the second pass's keys in the first pass's order
static __global__ void __launch_bounds__(LQ_POL_THREADS)
k_pol_rekey(const u64 *k_zs, const u64 *idx, u64 n, u64 *k2)
{
	for (u64 i = (u64)blockIdx.x * LQ_POL_THREADS + threadIdx.x; i < n; i += (u64)gridDim.x * LQ_POL_THREADS) k2[i] = k_zs[idx[i]];
}

// flag has n + 1 entries; n: the items that are not void (they sort in front)
static __global__ void __launch_bounds__(LQ_POL_THREADS)
k_pol_order(const PolItem *items, const u64 *key, const u64 *idx, u64 n, PolItem *sorted, u32 *flag)
{
	for (u64 i = (u64)blockIdx.x * LQ_POL_THREADS + threadIdx.x; i <= n; i += (u64)gridDim.x * LQ_POL_THREADS) {
		if (i == n) { flag[i] = 0; continue; }
		sorted[i] = items[idx[i]];
		flag[i] = i == 0 || (u32)(key[i - 1] >> 32) != (u32)(key[i] >> 32) ? 1u : 0u;
	}
}

// pos: the exclusive scan of flag over n + 1 entries (pos[n] = the ZMWs); head has pos[n] + 1 entries
static __global__ void __launch_bounds__(LQ_POL_THREADS)
k_pol_heads(const u32 *flag, const u32 *pos, u64 n, u32 *head)
{
	for (u64 i = (u64)blockIdx.x * LQ_POL_THREADS + threadIdx.x; i < n; i += (u64)gridDim.x * LQ_POL_THREADS) {
		if (flag[i]) head[pos[i]] = (u32)i;
		if (i + 1 == n) head[pos[n]] = (u32)n;
	}
}

// construct_polread (lq_sequel.py:76-137) over s[0 .. n), one ZMW's items in their order, without its two strings
__host__ __device__ __forceinline__ void lq_pol_walk_one(const PolItem *s, u32 n, i64 *hq_out, i64 *tot_out, u32 *ad_out, u32 *pol_out)
{
	i64 prev_end = 0, hs = -1, he = -1, hq = 0, tot = 0;
	u32 ad = 0, pol = 0;
	for (u32 k = 0; k < n; ++k) {
		const PolItem it = s[k];
		const i64 b = it.start, e = it.end;
		if (prev_end != 0 && prev_end != b) {                    // a gap is charged (it may be negative: items that overlap)
			const i64 gap = b - prev_end - 1;
			if (hs >= 0) hq -= gap;
			tot += gap;
		}
		prev_end = e;
		if (it.cls == 'L') {
			if (hs >= 0) { hq += he - hs; hs = he = -1; }
		} else {
			if (hs < 0) hs = b;
			he = e;
			if (it.cls == 'S') pol = 1;
			else if (it.cls == 'A') ++ad;
		}
		tot += e - b;
	}
	if (hs >= 0) hq += he - hs;
	if (hq > 0) ++hq;
	++tot;
	*hq_out = hq; *tot_out = tot; *ad_out = ad; *pol_out = pol;
}

// list == nullptr: ZMW g of n_zmw, those of more than LQ_POL_LONG items appended to long_list (n_long counts them) and left out;
// else: the ZMWs list[0 .. n_zmw).  pol[g]: bit 0 is_pol, bit 1 is_pol with tot == 0 (the reference divides by it), bit 2 is_pol with hq or
// tot outside uint32
static __global__ void __launch_bounds__(LQ_POL_THREADS)
k_pol_walk(const PolItem *sorted, const u32 *head, u64 n_zmw, const u32 *list, u32 *long_list, u32 *n_long,
           u32 *zmw, i64 *hq, i64 *tot, u32 *ad, u32 *pol)
{
	for (u64 j = (u64)blockIdx.x * LQ_POL_THREADS + threadIdx.x; j < n_zmw; j += (u64)gridDim.x * LQ_POL_THREADS) {
		const u32 g = list ? list[j] : (u32)j;
		const u32 h0 = head[g], cnt = head[g + 1] - h0;
		if (!list && cnt > LQ_POL_LONG) { long_list[atomicAdd(n_long, 1u)] = g; continue; }
		i64 q, t; u32 a, p;
		lq_pol_walk_one(sorted + h0, cnt, &q, &t, &a, &p);
		if (p && t == 0) p |= 2u;
		if (p && (q < 0 || q > 0xffffffffLL || t < 0 || t > 0xffffffffLL)) p |= 4u;
		zmw[g] = sorted[h0].zmw; hq[g] = q; tot[g] = t; ad[g] = a; pol[g] = p;
	}
}

// isp[g] = pol[g] & 1 for the scan (n_zmw + 1 entries, the last 0)
static __global__ void __launch_bounds__(LQ_POL_THREADS)
k_pol_ispol(const u32 *pol, u64 n_zmw, u32 *isp)
{
	for (u64 g = (u64)blockIdx.x * LQ_POL_THREADS + threadIdx.x; g <= n_zmw; g += (u64)gridDim.x * LQ_POL_THREADS) isp[g] = g < n_zmw ? pol[g] & 1u : 0u;
}

// the host sets sums to {0, 0, ~0, 0, 0, 0, ~0, 0, 0, 0}
static __global__ void __launch_bounds__(LQ_POL_THREADS)
k_pol_pack(const i64 *hq, const i64 *tot, const u32 *ad, const u32 *pol, const u32 *pos, u64 n_zmw, u32 *hq32, u32 *tot32, u32 *ad32, u32 *key, PolSums *sums)
{
	__shared__ u64 wsum[LQ_POL_THREADS / 64];
	u64 sum = 0, mx = 0, tmin = LQ_U64MAX, tmax = 0, nf = 0, nr = 0;
	u32 amin = 0xffffffffu, amax = 0;
	for (u64 g = (u64)blockIdx.x * LQ_POL_THREADS + threadIdx.x; g < n_zmw; g += (u64)gridDim.x * LQ_POL_THREADS) {
		const u32 p = pol[g];
		if (!(p & 1u)) continue;
		nf += p >> 1 & 1; nr += p >> 2 & 1;
		const u32 at = pos[g], a = ad[g];
		const u64 q = p & 4u ? 0 : (u64)hq[g], t = p & 4u ? 0 : (u64)tot[g];
		hq32[at] = (u32)q; tot32[at] = (u32)t; ad32[at] = a; key[at] = ~(u32)q;
		sum += q; mx = q > mx ? q : mx; tmin = t < tmin ? t : tmin; tmax = t > tmax ? t : tmax;
		amin = a < amin ? a : amin; amax = a > amax ? a : amax;
	}
	for (int o = 1; o < 64; o <<= 1) {                            // (every lane of the block is here: the loop above has no collective)
		const u64 m = __shfl_xor(mx, o), lo = __shfl_xor(tmin, o), hi = __shfl_xor(tmax, o);
		const u32 al = __shfl_xor(amin, o), ah = __shfl_xor(amax, o);
		mx = m > mx ? m : mx; tmin = lo < tmin ? lo : tmin; tmax = hi > tmax ? hi : tmax; amin = al < amin ? al : amin; amax = ah > amax ? ah : amax;
	}
	u64 s_all, f_all, r_all;
	lq_fx_block_scan(sum, wsum, &s_all);
	lq_fx_block_scan(nf, wsum, &f_all);
	lq_fx_block_scan(nr, wsum, &r_all);
	if ((threadIdx.x & 63) == 0 && tmin <= tmax) {
		atomicMax(&sums->max_hq, (unsigned long long)mx); atomicMin(&sums->min_tot, (unsigned long long)tmin); atomicMax(&sums->max_tot, (unsigned long long)tmax);
		atomicMin(&sums->min_ad, amin); atomicMax(&sums->max_ad, amax);
	}
	if (threadIdx.x == 0) {
		if (s_all) atomicAdd(&sums->sum_hq, (unsigned long long)s_all);
		if (f_all) atomicAdd(&sums->n_flagged, (unsigned long long)f_all);
		if (r_all) atomicAdd(&sums->n_range, (unsigned long long)r_all);
	}
}

static __global__ void __launch_bounds__(LQ_POL_THREADS)
k_pol_unkey(const u32 *k, u64 n, u32 *v)
{
	for (u64 i = (u64)blockIdx.x * LQ_POL_THREADS + threadIdx.x; i < n; i += (u64)gridDim.x * LQ_POL_THREADS) v[i] = ~k[i];
}

// v descending, ex its exclusive scan, sums->sum_hq their sum: the one index at which each comparison turns true writes its value
static __global__ void __launch_bounds__(LQ_POL_THREADS)
k_pol_nxx(const u32 *v, const u64 *ex, u64 n, PolSums *sums)
{
	const u64 sum = sums->sum_hq;
	for (u64 i = (u64)blockIdx.x * LQ_POL_THREADS + threadIdx.x; i < n; i += (u64)gridDim.x * LQ_POL_THREADS) {
		const u64 before = ex[i], with = before + v[i];
		if (2 * with >= sum && (i == 0 || 2 * before < sum)) sums->n50 = v[i];
		if (100 * with >= 90 * sum && (i == 0 || 100 * before < 90 * sum)) sums->n90 = v[i];
	}
}
