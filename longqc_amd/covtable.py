"""The output contract of the path as its consumer reads it: the 9-column table
`minimap2-coverage` prints, parsed the way LongQC's `LqCoverage` parses it (lq_coverage.py:87-107: tab-separated,
no header, columns 3 and 4 kept as text, spike-in control reads dropped by name), and the figures that are exact
functions of the table (lq_coverage.py:211-224).  Constructing a table is pure numpy and touches no device.  What follows in the
reference runs on request: est_coverage() makes the coverage estimate of lq_coverage.py:227-284 with both mixture fits on the device
(mixfit.gmm2 from a deterministic start in place of sklearn's seeded k-means, mixfit.lognorm_norm for mixEM's normal + log-normal
fit) and the reference's getters, calc_xome_size() and json_block() report it; coverage_dist_data(), outlier_data() and
terminal_data() are the numbers behind its remaining figures, bootstrap_main() refits resamples in one launch.  The numbers behind
its two grouped box plots, length_vs_coverage_data() and qscore_data() (lq_coverage.py:438-529), run on the device through
figdata.box_stats.

Same names as the reference where one exists: get_unmapped_frac(), get_unmapped_med_frac(), get_high_div_frac(),
get_control_num(), get_control_frac(), get_mean(), get_sd(), get_logn_mode(), get_logn_mu(), get_logn_sigma(),
get_expected_zero_rate(), is_no_coverage(), is_low_coverage(), get_warnings(), get_errors() (lq_coverage.py:125-209).
"""
from __future__ import annotations

import math
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
        """the table's rows; path: a file's name, or an open text file (an io.StringIO of a table held in memory)"""
        if hasattr(path, "read"):
            return [l.rstrip("\n").split("\t") for l in path if l.strip()]
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
        sigma lines and the outlier check on these medians: outlier_data()"""
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

    # ---- the coverage estimate: what LqCoverage.__est_coverage does after the fractions (lq_coverage.py:227-284) ---------------------
    UNMAPPED_FRACTION_THRESHOLD = 0.4  # lq_coverage.py:69-72
    UNMAPPED_FRACTION_PARAM_MIN = 0.05
    UNMAPPED_FRACTION_PARAM_MAX = 0.2
    COV_CORRECTION = 0.9
    # the reference's fields before its estimation; est_coverage() sets them on the instance
    model = mean_main = cov_main = main_comp_index = low_coverage = no_coverage = min_lambda = max_lambda = None
    mix_model = mode_logn_main = mu_logn_main = sigma_logn_main = raw_hist = selected = None
    is_transcript = False
    warnings = errors = ()

    def selected_coverage(self) -> np.ndarray:
        """the values both fits see (lq_coverage.py:579-583, 554-557): the non-zero values of column 8 strictly below its 0.85 quantile
        (pandas': np.percentile's linear rule with NaN left out), below its maximum when that quantile is 0.0; a "-nan" drops out"""
        known = self.cov[~np.isnan(self.cov)]
        th = float(np.percentile(known, 0.85 * 100)) if known.size else math.nan
        if th == 0.0:
            th = float(np.percentile(known, 1.0 * 100))
        with np.errstate(invalid="ignore"):
            return self.cov[(self.cov != 0) & (self.cov < th)]

    @staticmethod
    def relative_maxima(h) -> np.ndarray:
        """scipy.signal.argrelmax(h)[0]: the places strictly greater than both neighbours, the two ends never"""
        h = np.asarray(h, dtype=np.float64)
        if h.size < 3:
            return np.zeros(0, dtype=np.int64)
        with np.errstate(invalid="ignore"):
            return np.flatnonzero((h[1:-1] > h[:-2]) & (h[1:-1] > h[2:])) + 1

    def _bin_edges(self):
        if not self.mean_main > 0 or not math.isfinite(self.mean_main + self.cov_main):
            raise ValueError("the main component's mean %r is not positive: no bin step" % (self.mean_main,))
        return np.arange(0, self.mean_main + 10 * np.sqrt(self.cov_main) + self.mean_main / 10, self.mean_main / 10)

    def _raw_histogram(self):
        """(density, edges): the histogram of n_mbase / qlen that the low-coverage verdict reads (lq_coverage.py:234-240)"""
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.histogram(self.n_mbase / self.qlen, bins=self._bin_edges(), density=True)

    def _fit_lognorm(self, device, lib):
        """__est_coverage_dist_lognorm_norm (lq_coverage.py:552-566): mix_model = (weights, mus, sigmas), component 0 the background normal"""
        from . import mixfit
        i_m = self.main_comp_index
        i_bg = i_m ^ 1
        start = (self.model["mu"][i_bg], np.sqrt(self.model["var"][i_bg]), np.log(self.model["mu"][i_m]), 1)
        if not all(math.isfinite(float(v)) for v in start):
            raise ValueError("the main component's mean %r has no logarithm" % (self.model["mu"][i_m],))
        fit = mixfit.lognorm_norm(self.selected, start, max_iter=500, device=device, lib=lib)
        self.mix_fit = fit
        self.mix_model = (fit["w"], [fit["mu"][0], fit["mu"][1]], [fit["sigma"][0], fit["sigma"][1]])

    def est_coverage(self, is_transcript=False, device: int = 0, lib=None):
        """The coverage estimate of LqCoverage (lq_coverage.py:227-284) with both mixture fits on the device (mixfit.gmm2,
        mixfit.lognorm_norm): sets the reference's fields (model: the Gaussian fit as mixfit.gmm2 returns it, mean_main, cov_main,
        main_comp_index, raw_hist = (density, edges), low_coverage, no_coverage, min_lambda, max_lambda, mix_model, mode_logn_main,
        mu_logn_main, sigma_logn_main) for the getters below and returns self.  The Gaussian fit starts from the best split of the sorted
        values, not from a seeded k-means: one result per table.  ValueError where the reference crashes: one selected value, selected
        values without variance, more than mixfit.MAX_N of them, a main mean that is not positive"""
        from . import mixfit
        self.is_transcript = bool(is_transcript)
        self.warnings, self.errors = [], []
        self.model = self.mix_model = self.mode_logn_main = self.mu_logn_main = self.sigma_logn_main = None
        self.min_lambda = self.max_lambda = self.low_coverage = self.no_coverage = None
        self.selected = sel = self.selected_coverage()
        if sel.size == 0:
            self.mean_main, self.cov_main, self.main_comp_index = 1, 10, 0           # the reference's dummy (lq_coverage.py:586)
        else:
            if sel.size < 2:
                raise ValueError("one selected coverage value: two components cannot be fitted")
            if sel.min() == sel.max():
                raise ValueError("the selected coverage values have no variance")
            if sel.size > mixfit.MAX_N:
                raise ValueError("%d selected coverage values: a fit takes at most %d" % (sel.size, mixfit.MAX_N))
            self.model = mixfit.gmm2(sel, device=device, lib=lib)
            self.main_comp_index = mixfit.main_component(self.model)
            self.mean_main = float(self.model["mu"][self.main_comp_index])
            self.cov_main = float(self.model["var"][self.main_comp_index])
        self.raw_hist = self._raw_histogram()
        with np.errstate(invalid="ignore", divide="ignore"):
            self.low_coverage = self._looks_lowcoverage(self.raw_hist[0])
        if self.unmapped_frac_med >= self.UNMAPPED_FRACTION_THRESHOLD:
            self.min_lambda = -1 * math.log(self.unmapped_frac_med - self.UNMAPPED_FRACTION_PARAM_MIN)
            self.max_lambda = -1 * math.log(self.unmapped_frac_med - self.UNMAPPED_FRACTION_PARAM_MAX)
        if self.model is None:
            self.low_coverage = None
            self.no_coverage = True
            return self
        if self.is_transcript or self.low_coverage:                 # the three cases of lq_coverage.py:259-284: one fit, the mode by the kind
            self._fit_lognorm(device, lib)
            mu, sigma = self.mix_model[1][1], self.mix_model[2][1]
            self.mode_logn_main = np.exp(mu - sigma ** 2 * 0.5) if self.is_transcript else np.exp(mu - sigma ** 2)
            self.mu_logn_main, self.sigma_logn_main = mu, sigma
        return self

    def _looks_lowcoverage(self, h) -> bool:
        """lq_coverage.py:287-295"""
        if h[0] / np.sum(h) < 0.01:
            return False
        return not any(h[i] > (h[0] / 5) for i in self.relative_maxima(h))

    def get_mean(self):
        return self.mean_main

    def get_sd(self):
        return np.sqrt(self.cov_main) if self.cov_main is not None else None

    def get_logn_mode(self):
        return self.mode_logn_main if self.mode_logn_main else None

    def get_logn_mu(self):
        return self.mu_logn_main

    def get_logn_sigma(self):
        return self.sigma_logn_main

    def get_expected_zero_rate(self):
        if not self.mode_logn_main and not self.mean_main:
            return None
        if not self.mode_logn_main:
            return (self.mean_main, 1.3865 * 0.64086 ** self.mean_main)
        return (self.mode_logn_main, 1.3865 * 0.64086 ** self.mode_logn_main)

    def is_no_coverage(self):
        return self.no_coverage

    def is_low_coverage(self):
        return self.low_coverage

    def get_errors(self):
        return self.errors

    def get_warnings(self):
        return self.warnings

    def calc_xome_size(self, throughput):
        """lq_coverage.py:368-386, the same strings"""
        if self.no_coverage:
            return "N/A"
        if self.is_transcript or self.low_coverage:
            m_size = int((throughput * (1.0 - self.unmapped_frac_med)) / self.mode_logn_main)
        else:
            m_size = int((throughput * (1.0 - self.unmapped_frac_med)) / self.mean_main)
        if self.unmapped_frac_med >= self.UNMAPPED_FRACTION_THRESHOLD:
            s1 = throughput * self.COV_CORRECTION * (1 - self.UNMAPPED_FRACTION_PARAM_MIN) / self.min_lambda
            s2 = throughput * self.COV_CORRECTION * (1 - self.UNMAPPED_FRACTION_PARAM_MAX) / self.max_lambda
            return "%d (e = %.1f%%), %d (e = 20%%), %d (e = 5%%)" % (m_size, self.unmapped_frac_med * 100, s2, s1)
        return "%d (e = %.1f%%)" % (m_size, self.unmapped_frac_med * 100)

    def json_block(self, throughput) -> dict:
        """the Coverage_stats entries of the run's JSON (longQC.py:659-681), after est_coverage()"""
        out = {"Estimated non-sense read fraction": float(self.get_unmapped_med_frac())}
        if self.get_control_frac():
            out["Estimated spiked-in control read fraction"] = float(self.get_control_frac())
        if self.is_transcript or self.is_low_coverage():
            out["Mode_coverage"] = float(self.get_logn_mode())
            out["mu_coverage"] = float(self.get_logn_mu())
            out["sigma_coverage"] = float(self.get_logn_sigma())
        elif self.is_no_coverage():
            out["Mean_coverage"] = out["SD_coverage"] = "NA"
        else:
            out["Mean_coverage"] = float(self.get_mean())
            out["SD_coverage"] = float(self.get_sd())
        out["Estimated crude Xome size"] = str(self.calc_xome_size(throughput))
        return out

    def outlier_data(self, interval=3000.0, device: int = 0, lib=None) -> dict:
        """The 3 sigma lines of plot_length_vs_coverage and the check of __check_outlier_coverage (lq_coverage.py:485-494, 517-525), after
        est_coverage(): "lines" (mean - 3 sd, mean + 3 sd), or None where the reference draws none (a lambda or a log-normal fit exists);
        "outliers": the reliable length bins whose median of column 8 lies above the upper line or at or below the lower one -- if there
        is one, the reference's warning is added to get_warnings()"""
        if self.min_lambda or self.max_lambda or self.mix_model is not None:
            return {"lines": None, "outliers": np.zeros(0, dtype=np.uint32), "warning": False}
        data = self.length_vs_coverage_data(interval, device, lib)
        lo, hi = self.get_mean() - 3 * self.get_sd(), self.get_mean() + 3 * self.get_sd()
        meds = data["median"][data["reliable"]]
        with np.errstate(invalid="ignore"):
            out = data["group"][data["reliable"]][(meds > hi) | (meds <= lo)]
        note = ("Coverage warning", "Coverage might not be homogenous over the read length.")
        if out.size and note not in self.warnings:
            self.warnings = list(self.warnings) + [note]
        return {"lines": (lo, hi), "outliers": out, "warning": bool(out.size)}

    def coverage_dist_data(self) -> dict:
        """What plot_coverage_dist computes before it draws (lq_coverage.py:297-354), after est_coverage(): "edges" and "density", the
        histogram of column 8; "x", the 5000-point grid, and "y", the fitted curve on it ("model": "lognorm" for the normal + log-normal
        mixture, "gmm" for the two Gaussians, None with y None where the estimate was skipped); "poisson": None or (k, pmf at min_lambda,
        pmf at max_lambda).  numpy and math.lgamma only"""
        edges = self._bin_edges()
        density = np.histogram(self.cov, bins=edges, density=True)[0]
        sd = np.sqrt(self.cov_main)
        x = np.linspace(0, self.mean_main + 10 * sd, 5000)
        norm = lambda mu, s: np.exp(-((x - mu) / s) ** 2 / 2) / (math.sqrt(2 * math.pi) * s)
        kind = y = None
        if self.mix_model is not None:
            w, mu, sg = self.mix_model
            kind, logn = "lognorm", np.zeros_like(x)
            pos = x > 0
            logn[pos] = np.exp(-(np.log(x[pos]) - mu[1]) ** 2 / (2 * sg[1] ** 2)) / (x[pos] * sg[1] * math.sqrt(2 * math.pi))
            y = w[0] * norm(mu[0], sg[0]) + w[1] * logn
        elif self.model is not None:
            kind = "gmm"
            y = sum(self.model["w"][k] * norm(self.model["mu"][k], math.sqrt(self.model["var"][k])) for k in (0, 1))
        poisson = None
        if self.min_lambda and self.max_lambda:
            k = np.arange(int(self.mean_main + 4 * sd) + 1)
            lg = np.array([math.lgamma(v + 1.0) for v in k.tolist()])
            poisson = (k, np.exp(k * math.log(self.min_lambda) - self.min_lambda - lg), np.exp(k * math.log(self.max_lambda) - self.max_lambda - lg))
        return {"edges": edges, "density": density, "x": x, "y": y, "model": kind, "poisson": poisson}

    def terminal_data(self, x_max=145) -> dict:
        """__region_analysis(3, 1) (lq_coverage.py:623-655) and the two histograms of plot_unmapped_frac_terminal over np.arange(0, x_max, 5):
        per read with coordinates in column 3 the start of its first region ("t5") and its length minus the end of its last ("t3"), the
        regions sorted; "internal": the gaps between neighbouring regions in the order they are written.  Integers, pure numpy"""
        t5, t3, internal = [], [], []
        for text, ql in zip(self.good_coords, self.qlen.tolist()):
            if text == "0":
                continue
            regs = [(int(r.split("-")[0]), int(r.split("-")[1])) for r in text.split(",")]
            ordered = sorted(regs)
            internal.extend(regs[k + 1][0] - regs[k][1] for k in range(len(regs) - 1))
            t5.append(ordered[0][0])
            t3.append(int(ql) - ordered[-1][1])
        edges = np.arange(0, x_max, 5)
        return {"t5": t5, "t3": t3, "internal": internal, "edges": edges, "hist5": np.histogram(np.array(t5, dtype=np.int64), bins=edges)[0],
                "hist3": np.histogram(np.array(t3, dtype=np.int64), bins=edges)[0]}

    def bootstrap_main(self, nbs=1000, seed=0, device: int = 0, lib=None) -> dict:
        """What the reference's abandoned est_confidence_interval_mu was after (lq_coverage.py:36-65), with all refits in one launch: nbs
        resamples of the selected values (seed: what np.random.default_rng takes, a Generator included; its integers() draws the rows),
        all fitted by one mixfit.gmm2_many call -> "mean" and "sd" of every replicate's main component and "mean_ci" / "sd_ci", their 0.5
        and 99.5 percentiles.  ValueError as est_coverage raises it, and for a resample without variance"""
        from . import mixfit
        sel = self.selected if self.selected is not None else self.selected_coverage()
        if sel.size < 2 or sel.size > mixfit.MAX_N:
            raise ValueError("%d selected coverage values: a fit takes 2 to %d" % (sel.size, mixfit.MAX_N))
        samples = sel[np.random.default_rng(seed).integers(0, sel.size, size=(int(nbs), sel.size))]
        if (samples.min(axis=1) == samples.max(axis=1)).any():
            raise ValueError("a resample without variance")
        fits = mixfit.gmm2_many(list(samples), device=device, lib=lib)
        main = [mixfit.main_component(f) for f in fits]
        mean = np.array([f["mu"][k] for f, k in zip(fits, main)])
        sd = np.sqrt(np.array([f["var"][k] for f, k in zip(fits, main)]))
        return {"mean": mean, "sd": sd, "mean_ci": tuple(np.percentile(mean, [0.5, 99.5])), "sd_ci": tuple(np.percentile(sd, [0.5, 99.5]))}

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
