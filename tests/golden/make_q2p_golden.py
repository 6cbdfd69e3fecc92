#!/usr/bin/env python3
"""Makes tests/golden/q2p_literals.json: the 127 entries of the reference's meanQ lookup table q2p[] (lqutils.c), read as
data, so that tests/test_oracle_vs_ref.py can compare the table the oracle and the product rebuild numerically with them.

    python tests/golden/make_q2p_golden.py <the reference's minimap2-coverage directory>/lqutils.c
"""
import json
import os
import re
import sys


def main():
    txt = open(sys.argv[1]).read()
    block = txt[txt.rindex("double q2p[] = {"):]
    block = block[:block.index("};")]
    lits = re.findall(r"\d\.\d{15}", block)
    assert len(lits) == 127, len(lits)
    out = os.path.join(os.path.dirname(os.path.abspath(__file__)), "q2p_literals.json")
    json.dump({"what": "q2p[0..126] of the reference's lqutils.c as printed there (15 decimals), index = phred quality", "literals": lits},
              open(out, "w"), indent=0)
    print("%s: %d entries" % (out, len(lits)))


if __name__ == "__main__":
    main()
