"""Writes tests/golden/boxstats.json: small grouped arrays of printed "%.3f" numbers (integer thousandths) and, per group, what LongQC's
box plots compute from them -- matplotlib.cbook.boxplot_stats(x, whis=1.5) on the group's non-missing values and pandas'
groupby(...).median().  tests/test_boxstats.py compares its numpy restatement and the device with these numbers where matplotlib and
pandas are not installed.  Data only.  Run with matplotlib and pandas importable:  python tests/golden/make_boxstats_golden.py"""
import json
import os

import matplotlib
import numpy as np
import pandas as pd
from matplotlib import cbook

MISSING = -2 ** 31
HERE = os.path.dirname(os.path.abspath(__file__))


def cases():
    rng = np.random.default_rng(18)
    out = []

    def case(name, groups, interval=0.0):
        """groups: [(key, [thousandths ...])]; the elements are shuffled so that no group arrives in order"""
        key = np.array([k for k, vals in groups for _ in vals], dtype=np.int64)
        thou = np.array([v for _, vals in groups for v in vals], dtype=np.int64)
        p = rng.permutation(key.shape[0])
        out.append({"name": name, "interval": interval, "whis": 1.5, "key": key[p].tolist(), "thou": thou[p].tolist()})

    case("sizes 1 2 3 4 5 8 9", [(g, rng.integers(0, 40000, n).tolist()) for g, n in enumerate((1, 2, 3, 4, 5, 8, 9))])
    case("sizes again, other values", [(g, rng.integers(5000, 9000, n).tolist()) for g, n in enumerate((9, 8, 5, 4, 3, 2, 1))])
    case("pairs", [(g, rng.integers(0, 60000, 2).tolist()) for g in range(12)])
    case("ties and all equal", [(0, [5, 5, 7, 7, 7, 9]), (1, [3000] * 6), (2, [12345]), (3, [7000, 7000]), (4, [1, 1, 1, 2, 2, 2, 2, 50])])
    case("the whisker falls back to the quartile", [(0, [0, 0, 0, 100000]), (1, [0, 100000, 100000, 100000])])
    case("one far outlier on each side", [(0, [-50000, 1000, 1100, 1200, 1300, 1400, 90000]), (1, [9000, 9100, 9150, 9200, 9300, 200000]),
                                          (2, [-200000, 9000, 9100, 9150, 9200, 9300])])
    case("negative values", [(0, [-3000, -2500, -10, 0, 15, -7]), (1, [-1, -2, -3, -4, -5, -6, -7, -8, -900]), (2, [-2147483647, 2147483646])])
    case("missing values", [(0, [MISSING, MISSING]), (1, [MISSING, 1000, MISSING, 2000, 3000]), (2, [MISSING]), (3, [4000, MISSING]), (5, [1, 2, 3])])
    case("group ids in every key byte", [(g, rng.integers(0, 20000, n).tolist()) for g, n in ((0, 3), (1, 4), (300, 5), (70000, 2), (2 ** 31, 6))])
    for interval in (3000.0, 1234.5, 7.0, 49.0):
        lens = np.concatenate([rng.integers(0, 30001, 24), np.arange(0, 30001, 49)[1:600:20], [0, 30000]])
        case("length bins, interval %r" % interval, [(int(l), [int(rng.integers(0, 45000))]) for l in lens], interval)
    return out


def main():
    res = []
    for c in cases():
        key, thou = np.array(c["key"], dtype=np.int64), np.array(c["thou"], dtype=np.int64)
        v = np.where(thou == MISSING, np.nan, thou / 1000)
        g = np.floor(key / c["interval"]) if c["interval"] else key
        df = pd.DataFrame({"g": g, "v": v})
        med = df.groupby("g")["v"].median()
        boxes = []
        for gid, sub in df.groupby("g"):
            x = sub["v"].dropna().values                              # (pandas drops NaN before matplotlib sees the column)
            b = {"group": int(gid), "n_all": int(sub.shape[0]), "n": int(x.shape[0])}
            if x.shape[0]:
                st = cbook.boxplot_stats(x, whis=c["whis"])[0]
                b.update({k: float(st[k]) for k in ("q1", "med", "q3", "whislo", "whishi")})
                b["fliers"] = sorted(float(f) for f in st["fliers"])
                b["median"] = float(med[gid])
                assert b["median"] == float(np.median(x))
            else:
                b.update({k: None for k in ("q1", "med", "q3", "whislo", "whishi", "median")})
                b["fliers"] = []
                assert np.isnan(med[gid])
            boxes.append(b)
        res.append(dict(c, boxes=boxes))
    doc = {"made_with": {"matplotlib": matplotlib.__version__, "pandas": pd.__version__, "numpy": np.__version__}, "missing": MISSING, "cases": res}
    with open(os.path.join(HERE, "boxstats.json"), "w") as f:
        json.dump(doc, f, separators=(",", ":"), allow_nan=False)
        f.write("\n")


if __name__ == "__main__":
    main()
