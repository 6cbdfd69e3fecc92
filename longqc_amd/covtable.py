"""The output contract of the path as its consumer reads it: the 9-column table
`minimap2-coverage` prints, parsed the way LongQC's `LqCoverage` parses it (lq_coverage.py:87-107: tab-separated,
no header, columns 3 and 4 kept as text, spike-in control reads dropped by name), and the figures that are exact
functions of the table (lq_coverage.py:211-224).  The mixture fits that follow in the reference are CPU
post-processing of <= 10 k rows with a random start and are not part of this build.  The numbers behind its two grouped box
plots are: length_vs_coverage_data() and qscore_data() (lq_coverage.py:438-529) run on the device through figdata.box_stats;
constructing a table and everything else stays pure numpy.

Same names as the reference where one exists: get_unmapped_frac(), get_unmapped_med_frac(), get_high_div_frac(),
get_control_num(), get_control_frac() (lq_coverage.py:160-203).
"""
from __future__ import annotations

from typing import List, Optional

import numpy as np


class CoverageTable:
    DIV_SCORE_THRESHOLD = 0.25         # lq_coverage.py:72
    COV_THRESHOLD_FOR_DIV_SC = 25      # lq_coverage.py:73
    LENGTH_BIN_THRESHOLD = 100         # lq_coverage.py:75
    MISSING = -2 ** 31                 # figdata.MISSING: a "-nan" among the thousandths
    # column numbers: lq_coverage.py:76-84
    READ_NAME_COLUMN, QLENGTH_COLUMN, N_MBASE_COLUMN, MED_READ_COV_CORS, T1_COVERAGE_COLUMN, QV_COLUMN, DIV_COLUMN, COVERAGE_COLUMN = 0, 1, 2, 4, 5, 6, 7, 8

    @staticmethod
    def _rows(path) -> List[List[str]]:
        with open(path) as f:
            return [l.rstrip("\n").split("\t") for l in f if l.strip()]

    def __init__(self, table_path, control_filtering: Optional[str] = None):
        rows = self._rows(table_path)
        self.control_reads = None
        if control_filtering is not None:
            self.control_reads = [r[0] for r in self._rows(control_filtering) if float(r[self.T1_COVERAGE_COLUMN]) >= 0.5]
            drop = set(self.control_reads)
            rows = [r for r in rows if r[0] not in drop]
        if not rows:
            raise ValueError("coverage table %s has no rows" % table_path)     # the reference divides by zero here
        if any(len(r) != 9 for r in rows):
            raise ValueError("coverage table %s: expected 9 tab-separated columns" % table_path)
        self.names = [r[0] for r in rows]
        self.qlen = np.array([int(r[1]) for r in rows], dtype=np.int64)
        self.n_mbase = np.array([int(r[2]) for r in rows], dtype=np.int64)
        self.good_coords = [r[3] for r in rows]
        self.med_coords = [r[4] for r in rows]
        self.t1_cov, self.qv, self.div, self.cov = (np.array([float(r[c]) for r in rows]) for c in (5, 6, 7, 8))
        self._printed = {c: [r[c] for r in rows] for c in (5, 6, 8)}       # the text of the columns the box plots read (thousandths)
        n = len(rows)
        med0 = np.array([c == "0" for c in self.med_coords])
        self.unmapped_frac_trimmed = int((self.t1_cov == 0.0).sum()) / n
        self.unmapped_frac_untrimmed = int((self.n_mbase == 0).sum()) / n
        self.unmapped_frac_med = int(med0.sum()) / n
        self.high_div_frac = int(((self.div >= self.DIV_SCORE_THRESHOLD) & (self.t1_cov >= self.COV_THRESHOLD_FOR_DIV_SC) & ~med0).sum()) / n

    @classmethod
    def _thou(cls, text) -> int:
        """a printed column 5 to 8 -> its integer thousandths: "0.0" is 0, "-nan" is MISSING, a sign is kept ("-0.000" is 0)"""
        if text.endswith("nan"):
            return cls.MISSING
        whole, _, frac = text.partition(".")
        if not frac.isdigit() or len(frac) > 3 or not whole.lstrip("-").isdigit():
            raise ValueError("coverage table: %r is not a %%.3f number" % (text,))
        v = int(whole.lstrip("-")) * 1000 + int(frac.ljust(3, "0"))
        if v >= 2 ** 31 - 1:
            raise ValueError("coverage table: %r does not fit 31 bits of thousandths" % (text,))
        return -v if whole.startswith("-") else v

    def thousandths(self, column) -> np.ndarray:
        """column 5, 6 or 8 as the integer thousandths its text shows (minimap2-coverage.c:587-604 prints "%.3f" or the literal 0.0), int32,
        "-nan" as MISSING: value / 1000 is the double pandas parses.  Pure numpy; a text of another form raises ValueError"""
        if not isinstance(self._printed[column], np.ndarray):
            self._printed[column] = np.array([self._thou(t) for t in self._printed[column]], dtype=np.int32)
        return self._printed[column]

    def length_vs_coverage_data(self, interval=3000.0, device: int = 0, lib=None) -> dict:
        """What plot_length_vs_coverage computes before it draws (lq_coverage.py:462-529), on the device (figdata.box_stats): the reads
        binned by np.floor(qlen / interval); "boxes": matplotlib's box per bin of MERGED_COVERAGE (column 8 where qlen >= 3000, else
        column 5: lq_coverage.py:507-508); per bin "median" and "size" of column 8 as __check_outlier_coverage groups them (the median
        pandas', NaN left out; the size every row's) and "reliable" = size >= LENGTH_BIN_THRESHOLD; "group": the bins that occur.  The 3
        sigma lines need the mixture fits and are not part of this build"""
        from . import figdata
        if int(self.qlen.min()) < 0 or int(self.qlen.max()) >= 1 << 32:
            raise ValueError("a read length outside 32 bits")
        key = self.qlen.astype(np.uint32)
        cov_thou = self.thousandths(self.COVERAGE_COLUMN)
        merged = np.where(self.qlen >= 3000, cov_thou, self.thousandths(self.T1_COVERAGE_COLUMN)).astype(np.int32)
        boxes = figdata.box_stats(key, merged, float(interval), 1.5, device, lib)
        cov = figdata.box_stats(key, cov_thou, float(interval), 1.5, device, lib)
        return {"group": cov["group"], "boxes": boxes, "median": cov["median"], "size": cov["n_all"].astype(np.int64),
                "reliable": cov["n_all"] >= self.LENGTH_BIN_THRESHOLD}

    def qscore_data(self, device: int = 0, lib=None) -> dict:
        """What plot_qscore_dist computes before it draws (lq_coverage.py:438-460), on the device: matplotlib's box of column 6 for the
        reads whose column 8 == 0.0 (group 0, "Non-sense reads") and for those where it != 0.0 (group 1, "Normal reads"; a "-nan" coverage
        is != 0.0).  -> figdata.box_stats' dict; a group without reads is not listed, a "-nan" QV is left out of its box"""
        from . import figdata
        return figdata.box_stats((self.thousandths(self.COVERAGE_COLUMN) != 0).astype(np.uint32), self.thousandths(self.QV_COLUMN), 0.0, 1.5, device, lib)

    def __len__(self):
        return len(self.names)

    def get_unmapped_frac(self):
        return self.unmapped_frac_trimmed

    def get_unmapped_med_frac(self):
        return self.unmapped_frac_med

    def get_high_div_frac(self):
        return self.high_div_frac

    def get_control_num(self):
        return len(self.control_reads) if self.control_reads else 0

    def get_control_frac(self):
        if self.control_reads:
            return len(self.control_reads) / (len(self.control_reads) + len(self.names))
        return 0.0
