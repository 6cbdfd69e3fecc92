"""Host-side counterpart of the slice of `longQC.py sampleqc` that feeds and drives the coverage path
(SURVEY.md section 8(f)-2): building the query set (LongQC's seed-7 chunk reservoir), writing it as FASTQ,
the preset -> argv table, and the launch itself -- through the argv-compatible boundary or, without the
temporary FASTQ round trip, straight from memory through the C ABI.

Reference behaviour mirrored here (same names, argument meaning and order where a function exists there):
  subsample_from_chunk      lq_utils.py:371-411
  write_fastq               lq_utils.py:352-369
  replace_masked            longQC.py:369-406   (re-draw replacements for heavily masked subsample reads)
  coverage_argv             longQC.py:171-233 (presets), :438-446 (main call), :555-556 (spike-in call)
Reads are [name, seq, qual] lists like the reference's chunks (lq_utils.py:211-289).
"""
from __future__ import annotations

import os
import shlex
from typing import Iterable, List, Optional, Sequence

import numpy as np

# minimap2 parameters per preset: (-p for normal reads, -p for --short reads) -- longQC.py:171-220
PRESET_MED_SCORE = {
    "pb-rs2": (80, 60), "pb-sequel": (80, 60), "pb-hifi": (80, None),
    "ont-ligation": (160, 140), "ont-rapid": (160, 140), "ont-1dsq": (160, 140),
}
# adapters per preset: (adp5, adp3), None where the preset sets none -- longQC.py:171-216 (--adapter_5 / --adapter_3 override
# them there); the chunk loop hands them to cut_adapter (longqc_amd/adapter.py)
_PB_RS2_ADP = "ATCTCTCTCTTTTCCTCCTCCTCCGTTGTTGTTGTTGAGAGAGAT"
_PB_SEQUEL_ADP = "ATCTCTCTCAACAACAACAACGGAGGAGGAGGAAAAGAGAGAGAT"
PRESET_ADAPTERS = {
    "pb-rs2": (_PB_RS2_ADP, _PB_RS2_ADP), "pb-sequel": (_PB_SEQUEL_ADP, _PB_SEQUEL_ADP), "pb-hifi": (_PB_SEQUEL_ADP, _PB_SEQUEL_ADP),
    "ont-ligation": ("AATGTACTTCGTTCAGTTACGTATTGCT", "GCAATACGTAACTGAACG"),
    "ont-rapid": ("GTTTTCGCATTTATCGTGAAACGCTTTCGCGTTTTTCGTGCGCCGCTTCA", None),
    "ont-1dsq": ("GGCGTCTGCTTGGGTGTTTAACCTTTTTGTCAGAGAGGTTCCAAGTCAGAGAGGTTCCT",
                 "GGAACCTCTCTGACTTGGAACCTCTCTGACAAAAAGGTTAAACACCCAAGCAGACGCCAGCAAT"),
}
MINIMAP2_PARAMS = "-Y -l 0 -q 160"                                      # longQC.py:177,186,194,202,209,217
MINIMAP2_FILTERING_PARAMS = "-Y -Hk15 -w 10 -c 1 -l 0 --filter"        # longQC.py:255 (spike-in control)


def db_params(preset: str, fast: bool = False, inds: str = "4G") -> str:
    """longQC.py:222-231"""
    if preset == "pb-hifi":
        return ("-k 19 -w 10 -I %s" if fast else "-k 15 -w 5 -I %s") % inds
    return ("-k 15 -w 5 -I %s" if fast else "-k 12 -w 5 -I %s") % inds


def coverage_argv(preset: str, fastx_path: str, sample_path: str, ncpu: int = 4, fast: bool = False, inds: str = "4G",
                  short: bool = False) -> List[str]:
    """The argv of the main minimap2-coverage call (longQC.py:443-445); short=True gives the --short variant
    (-k 12 -w 5 and the lower -p, longQC.py:447-... )."""
    if preset not in PRESET_MED_SCORE:
        raise ValueError("unknown preset %r" % preset)
    med, med_short = PRESET_MED_SCORE[preset]
    if short:
        if med_short is None:
            raise ValueError("--short is not defined for %s" % preset)
        return shlex.split("%s %s -p %d -t %d %s %s" % (MINIMAP2_PARAMS, "-k 12 -w 5 -I %s" % inds, med_short, ncpu, fastx_path, sample_path))
    return shlex.split("%s %s -p %d -t %d %s %s" % (MINIMAP2_PARAMS, db_params(preset, fast, inds), med, ncpu, fastx_path, sample_path))


def db_build_argv(preset: str, tempdb_path: str, fastx_path: str, fast: bool = False, inds: str = "4G", short: bool = False) -> List[str]:
    """`sampleqc --db`, first call: index every read into a prebuilt .mmi (longQC.py:266-277); short=True gives the
    t_db_minimap2_short variant (-k 12 -w 5).  With --db --short and equal index options (every preset but pb-hifi, without
    --fast) the two .mmi files are the same: one serves both subsamples, mapped in one call with lqcov_run_files_sets
    (Engine.run_files_sets: the main set with the preset's -p, the short set with the --short -p)."""
    params = "-k 12 -w 5 -I %s" % inds if short else db_params(preset, fast, inds)
    return shlex.split("%s -d %s %s" % (params, tempdb_path, fastx_path))


def db_coverage_argv(preset: str, tempdb_path: str, sample_path: str, ncpu: int = 4, short: bool = False) -> List[str]:
    """`sampleqc --db`, second call: map the subsample against the prebuilt index; no -k/-w on this command line
    (longQC.py:440-442, 531-533), so the binary sizes its counters with its defaults (k=12, w=5) while the index's
    own k / w drive the mapping."""
    if preset not in PRESET_MED_SCORE:
        raise ValueError("unknown preset %r" % preset)
    med, med_short = PRESET_MED_SCORE[preset]
    if short and med_short is None:
        raise ValueError("--short is not defined for %s" % preset)
    return shlex.split("%s -p %d -t %d %s %s" % (MINIMAP2_PARAMS, med_short if short else med, ncpu, tempdb_path, sample_path))


def spikein_argv(filter_ref: str, sample_path: str, ncpu: int = 4) -> List[str]:
    """longQC.py:555-556"""
    return shlex.split("%s -t %d %s %s" % (MINIMAP2_FILTERING_PARAMS, ncpu, filter_ref, sample_path))


def subsample_from_chunk(chunk, cum_n_seq, s_reads, param, s_seed=7, elist=None):
    """The draw of lq_utils.py:371-411 over one chunk of reads, all reads of the chunk at once.

    The reference's generator is re-seeded per chunk (seed 7) and draws len(chunk) + 1 uniforms; the k-th read that is not on
    `elist` uses the k-th of them.  param >= 1 keeps a reservoir of int(param) reads: the n-th read seen so far (over all
    chunks, n counted from 1) goes to slot n - 1 while the reservoir fills and to slot floor(u * n) afterwards, if that slot
    exists; of several reads aimed at one slot the last one stays.  param < 1 keeps a read when its uniform is below param."""
    take = [r for r in chunk if not (elist and r[0] in elist)]
    u = np.random.RandomState(s_seed).uniform(size=len(chunk) + 1)[:len(take)]
    if param < 1.:
        kept = np.flatnonzero(u < param)
        return s_reads + [[take[i][0], take[i][1], take[i][2]] for i in kept]
    size = int(param)
    if not s_reads:
        s_reads = [0] * size
    nth = cum_n_seq + 1 + np.arange(len(take), dtype=np.int64)
    slot = np.where(nth - 1 < size, nth - 1, (u * nth).astype(np.int64))
    hit = np.flatnonzero(slot < size)
    # the last read aimed at a slot wins: walk the hits backwards and keep the first sight of every slot
    _, first_from_back = np.unique(slot[hit][::-1], return_index=True)
    for i in hit[::-1][first_from_back]:
        s_reads[int(slot[i])] = [take[i][0], take[i][1], take[i][2]]
    return s_reads


def subsample_from_resident(chunk, cum_n_seq, s_reads, param, s_seed=7, elist=None):
    """subsample_from_chunk on a chunkpass.ReadChunk that lives on the device: the same slots from chunk.n, cum_n_seq and the same
    uniforms, `elist` applied to chunk.names; only the reads that end up in a slot are fetched (chunk.records(idx))."""
    names = chunk.names
    take = np.array([i for i in range(chunk.n) if not (elist and names[i] in elist)], dtype=np.int64)
    u = np.random.RandomState(s_seed).uniform(size=chunk.n + 1)[:take.shape[0]]
    if param < 1.:
        return s_reads + chunk.records(take[np.flatnonzero(u < param)])
    size = int(param)
    if not s_reads:
        s_reads = [0] * size
    nth = cum_n_seq + 1 + np.arange(take.shape[0], dtype=np.int64)
    slot = np.where(nth - 1 < size, nth - 1, (u * nth).astype(np.int64))
    hit = np.flatnonzero(slot < size)
    _, first_from_back = np.unique(slot[hit][::-1], return_index=True)
    win = hit[::-1][first_from_back]
    for i, r in zip(win.tolist(), chunk.records(take[win])):
        s_reads[int(slot[i])] = r
    return s_reads


def replace_masked(s_reads, exclude_seqs: Sequence[str], chunks: Iterable, logger=None):
    """longQC.py:369-406.  Reads of the subsample that sit on the highly-masked list are swapped for a second reservoir draw
    over the input -- one slot per masked read, skipping every read that was already picked or is masked itself.  The draw stops
    at the first chunk after which every slot is taken; if the input runs out first, the masked reads are dropped instead.
    `chunks` yields (reads, n_seqs, n_bases); reads: a list of records, or a chunkpass.ReadChunk on the device (a FileChunks)."""
    picked = [r for r in s_reads if r != 0]
    masked = set(exclude_seqs)
    where = [i for i, r in enumerate(picked) if r[0] in masked]
    if not where:
        return picked
    avoid = masked | {r[0] for r in picked}
    spare = [0] * len(where)
    seen = 0
    for reads, n_seqs, _n_bases in chunks:
        (subsample_from_resident if hasattr(reads, "records") else subsample_from_chunk)(reads, seen, spare, len(where), elist=avoid)
        seen += n_seqs
        if all(spare):
            break
    if not all(spare):
        gone = set(where)
        return [r for i, r in enumerate(picked) if i not in gone]
    for i, r in zip(where, spare):
        picked[i] = r
    return picked


def write_fastq(fn, reads, is_chunk=False):
    """lq_utils.py:352-369 (returns True on success, None when the file exists or there is nothing to write)"""
    if not is_chunk and os.path.isfile(fn):
        return None
    if len(reads) == 0:
        return None
    with open(fn, "a" if is_chunk else "w") as fq:
        for r in reads:
            fq.write("@%s\n%s\n+\n%s\n" % tuple(r))
    return True


def _to_arrays(reads):
    names = [r[0] for r in reads]
    seqs = [np.frombuffer(r[1].encode() if isinstance(r[1], str) else bytes(r[1]), dtype=np.uint8) for r in reads]
    quals = None
    if all(len(r) > 2 and r[2] for r in reads):
        quals = [np.frombuffer(r[2].encode() if isinstance(r[2], str) else bytes(r[2]), dtype=np.uint8) for r in reads]
    return names, seqs, quals


def short_split(s_reads, length_threshold: int = 500):
    """longQC.py:410-413: (reads of at least length_threshold bases, shorter reads), each in the subsample's order"""
    reads = [r for r in s_reads if r]
    return [r for r in reads if len(r[1]) >= length_threshold], [r for r in reads if len(r[1]) < length_threshold]


def coverage_in_memory(chunks: Iterable, s_reads, preset: str = "ont-ligation", fast: bool = False, inds: int = 4000000000,
                       out: Optional[str] = None, device: int = 0, engine=None, short: bool = False,
                       short_threshold: Optional[int] = None):
    """The same computation as `LqExec(minimap2-coverage).exec(*coverage_argv(...))` without writing
    subsample.fastq and re-parsing both files (minimap2-coverage.c:408,471 parse the query file twice): the
    subsample goes to the device once, the input chunks (`chunks` yields (reads, n_seqs, n_bases), reads =
    [name, seq, qual]) are streamed into index parts cut by the reference's rule (index.c:244,311-316).
    Returns the table text (also written to `out` if given).  short=True: the --short call's argv (coverage_argv).

    short_threshold (LongQC's --short, 500): s_reads is split as longQC.py:410-413 does (short_split) and both calls of
    longQC.py:438-445,527-543 are made -> (main table, short table); `out`, if given, gets their concatenation (LongQC's
    merged_coverage_out.txt).  Where the two calls index the targets alike (every preset but pb-hifi, without `fast`), the
    two sets are mapped in ONE pass over `chunks`, each with its own -p; otherwise `chunks` must be re-iterable (a list)."""
    if short_threshold is None:
        text = _coverage_pass(chunks, [(s_reads, coverage_argv(preset, "-", "-", fast=fast, inds=str(inds), short=short))], device, engine)[0]
    else:
        main_reads, short_reads = short_split(s_reads, short_threshold)
        argv_main = coverage_argv(preset, "-", "-", fast=fast, inds=str(inds))
        argv_short = coverage_argv(preset, "-", "-", fast=fast, inds=str(inds), short=True)     # (pb-hifi: raises, as the CLI has no --short -p)
        strip_p = lambda a: [x for i, x in enumerate(a) if x != "-p" and (i == 0 or a[i - 1] != "-p")]
        if strip_p(argv_main) == strip_p(argv_short):
            text = _coverage_pass(chunks, [(main_reads, argv_main), (short_reads, argv_short)], device, engine)
        else:
            if engine is not None:
                raise ValueError("two passes with different index options need two handles: pass engine=None")
            text = [_coverage_pass(chunks, [(main_reads, argv_main)], device, None)[0], _coverage_pass(chunks, [(short_reads, argv_short)], device, None)[0]]
        text = tuple(text)
    if out:
        with open(out, "w") as f:
            f.write(text if isinstance(text, str) else "".join(text))
    return text


def set_query_reads(eng, sets) -> None:
    """the queries of one pass over the targets: the reads of the one (reads, argv) of `sets`, or one query set per entry, each with
    the -p / -q of its argv"""
    from . import api
    if len(sets) == 1:
        qn, qs, qq = _to_arrays([r for r in sets[0][0] if r])
        eng.set_queries(qn, qs, qq)
        return
    qsets = []
    for reads, argv in sets:
        ps, _, _ = api.parse_args(argv)
        qn, qs, qq = _to_arrays([r for r in reads if r])
        qsets.append((qn, qs, qq, int(ps.min_score_med), int(ps.min_score_good)))
    eng.set_query_sets(qsets)


def _coverage_pass(chunks: Iterable, sets, device: int, engine) -> List[str]:
    """one pass over the target chunks for every (reads, argv) of `sets`; the argvs differ at most in -p -> one table per set"""
    from . import api
    p, _, _ = api.parse_args(sets[0][1])
    eng = engine or api.Engine(p, device=device)
    try:
        set_query_reads(eng, sets)
        batch = int(p.batch_size)
        mini = min(int(p.idx_mini_batch), batch)
        part, part_bases, pend, pend_bases = None, 0, [], 0

        def flush_minibatch():
            nonlocal part, part_bases, pend, pend_bases
            if not pend:
                return
            if part is None:
                part = eng.part_begin(); part_bases = 0
            tn, ts, _ = _to_arrays(pend)
            eng.part_add_targets(part, tn, ts)
            part_bases += pend_bases
            pend, pend_bases = [], 0

        def close_part():
            nonlocal part, part_bases
            if part is not None:
                eng.part_build(part); eng.part_map(part); eng.part_release(part)
            part, part_bases = None, 0

        for (reads, n_seqs, n_bases) in chunks:
            for r in reads:
                if not pend and part is not None and part_bases > batch:      # checked before each mini-batch (index.c:244)
                    close_part()
                pend.append(r); pend_bases += len(r[1])
                if pend_bases >= mini:                                          # a mini-batch ends with the read that reaches the size
                    flush_minibatch()
        flush_minibatch()
        close_part()
        eng.finish()
        if len(sets) == 1:
            return [eng.table_text()]
        return [eng.table_text(set=k) for k in range(len(sets))]
    finally:
        if engine is None:
            eng.close()
