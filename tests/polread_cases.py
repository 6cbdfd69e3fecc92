"""The inputs of the Sequel platform QC's golden cases (tests/golden/polread.json): item lists and runs made from seeds by the generator
below, so that the file holds only what the reference returned for them.  tests/golden/make_polread_golden.py builds the same inputs from
this module, hands them to the reference's functions and records the results; load() puts inputs and results together."""
import hashlib
import json
import os

M64 = (1 << 64) - 1
UNITS = {
    "issue_1": [(0, 100, "L"), (100, 150, "A"), (150, 1000, "S"), (1000, 1045, "A"), (1045, 2000, "S"), (2000, 2500, "L")],
    "issue_2": [(10, 100, "S"), (100, 100, "A"), (10, 100, "F")],
    "issue_3": [(0, 50, "L"), (60, 90, "F")],
    "issue_4": [(0, 50, "S"), (70, 90, "L"), (95, 120, "S")],
    "issue_5": [(5, 50, "S")],
    "issue_6": [(0, 0, "S")],
    "tie_L_first": [(0, 40, "S"), (40, 90, "L"), (40, 90, "A"), (90, 200, "S")],
    "tie_L_last": [(0, 40, "S"), (40, 90, "A"), (40, 90, "L"), (90, 200, "S")],
    "tie_L_first_only": [(40, 90, "L"), (40, 90, "S")],
    "tie_L_last_only": [(40, 90, "S"), (40, 90, "L")],
    "overlap": [(0, 100, "S"), (50, 150, "A"), (120, 300, "S"), (10, 20, "B")],
    "zero_then_gap": [(0, 0, "A"), (30, 80, "S"), (100, 140, "S")],
    "zero_end_mid": [(5, 0, "S"), (30, 80, "S")],
    "no_S": [(0, 100, "L"), (100, 150, "A"), (150, 400, "F")],
    "only_L": [(3, 9, "L")],
    "unknown_class": [(0, 10, "Q"), (10, 50, "S"), (50, 60, "B"), (60, 61, "A"), (61, 99, "F")],
    "reversed": [(100, 50, "S"), (50, 10, "A")],
    "large": [(999999000, 999999999, "S"), (0, 999999999, "A")],
}
N_RANDOM_UNITS = 200
# lengths a single item (0, v - 1, S) gives: 0, or 2 and more
NXX = [[5000], [7, 7, 7, 7, 7, 7], [2, 3, 4, 5, 6, 7, 8, 9, 10, 11], [10, 10, 2, 2, 2, 2, 2], [0, 0, 3], [0], [10 ** 9, 10 ** 9 - 1, 77, 3]]
RUNS = (("small", 40, False), ("main", 250, False), ("zero_hq", 30, True))       # name, ZMWs, one read of HQ length 0


class Rng:
    """a 64-bit linear congruential generator: the same numbers from every Python"""

    def __init__(self, seed):
        self.x = (seed * 0x9E3779B97F4A7C15 + 1) & M64

    def below(self, n):
        self.x = (self.x * 6364136223846793005 + 1442695040888963407) & M64
        return (self.x >> 33) % n

    def between(self, lo, hi):
        return lo + self.below(hi - lo + 1)

    def shuffle(self, l):
        for i in range(len(l) - 1, 0, -1):
            j = self.below(i + 1)
            l[i], l[j] = l[j], l[i]


def random_zmw(rng, classes="AABFLLSSSS"):
    """1..40 items: mostly a chain of touching intervals with the odd gap, overlap, repeat and (0, 0), in a shuffled arrival order"""
    n, pos, out = rng.between(1, 40), (0, 0, rng.between(0, 5000))[rng.below(3)], []
    for _ in range(n):
        r = rng.below(100)
        if r < 8:
            pos += rng.between(1, 300)
        elif r < 14:
            pos = max(0, pos - rng.between(1, 200))
        ln = (0, 1, rng.between(1, 60), rng.between(30, 9000))[rng.below(4)]
        out.append((pos, pos + ln, classes[rng.below(len(classes))]))
        if r >= 95:
            out.append((pos, pos + ln, classes[rng.below(len(classes))]))
        pos += ln
    rng.shuffle(out)
    return out


def units():
    rng = Rng(7)
    return list(UNITS.items()) + [("random_%d" % i, random_zmw(rng)) for i in range(N_RANDOM_UNITS)]


def nxx_lists():
    rng = Rng(8)
    return NXX + [[rng.between(2, 60000) for _ in range(n)] for n in (2, 3, 64, 1000)]


def make_run(seed, n_zmw, with_zero_hq=False, movie="m54_1"):
    """-> (scraps records [name, sz, sc] (None: the tag is missing), subreads records [name]), each file in a shuffled order"""
    rng = Rng(seed)
    scraps, subreads, zmws = [], [], [4194369, 4194369 + (1 << 24), 4194369 + (1 << 25)]      # equal below bit 24
    while len(zmws) < n_zmw:
        z = rng.between(1, 40 * n_zmw)
        if z not in zmws:
            zmws.append(z)
    for k, z in enumerate(zmws):
        items = random_zmw(rng, "AABFLLSSSS" if k % 9 else "AABFLL")
        if with_zero_hq and k == 5:
            items = [(0, 0, "S")]
        for s, e, c in items:
            nm = "%s/%d/%d_%d" % (movie, z, s, e)
            if c == "S":
                subreads.append([nm])
            else:
                scraps.append([nm, "N", c])
        r = rng.below(10)
        if r < 3:                                                 # records that give no item
            scraps.append(["%s/%d/%d_%d" % (movie, z, rng.between(0, 900), rng.between(0, 90000)), "C", "FFFA"[rng.below(4)]])
        elif r < 4:
            scraps.append(["%s/%d/0_10" % (movie, z)] + list([(None, "A"), ("N", None), ("X", "A"), (None, None)][rng.below(4)]))
    rng.shuffle(scraps)
    rng.shuffle(subreads)
    return scraps, subreads


def digest(inputs):
    """what the golden file records of its inputs: they are made here from seeds, and the results belong to exactly these"""
    return hashlib.sha256(json.dumps(inputs, separators=(",", ":")).encode()).hexdigest()


def load():
    """-> {"units": [{name, items, expect}], "runs": [{name, scraps, subreads, expect}], "nxx": [{vals, n50, n90}], "zero_hq": {...}}"""
    g = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "polread.json")))
    out = {"zero_hq": g["zero_hq"], "units": [{"name": n, "items": [list(i) for i in items], "expect": g["units"][n]} for n, items in units()]}
    out["nxx"] = [{"vals": v, "n50": r[0], "n90": r[1]} for v, r in zip(nxx_lists(), g["nxx"])]
    out["runs"] = []
    for name, n, zero in RUNS:
        scraps, subreads = make_run(g["runs"][name]["seed"], n, zero)
        out["runs"].append({"name": name, "scraps": scraps, "subreads": subreads, "expect": g["runs"][name]["expect"]})
    assert len(out["units"]) == len(g["units"]) and len(out["nxx"]) == len(g["nxx"])
    got = {"units": digest([[n, [list(i) for i in items]] for n, items in units()]), "nxx": digest(nxx_lists())}
    got.update({r["name"]: digest([r["scraps"], r["subreads"]]) for r in out["runs"]})
    assert got == g["inputs_sha256"], "tests/polread_cases.py no longer makes the inputs tests/golden/polread.json was recorded for: run the generator"
    return out
