"""The record stage of the Sequel platform QC: k_pol_fields / k_pol_compact over the device record walk's rows (lqpol_fields), the host
twin (lqpol_twin) and the two together behind lqpol_add_bytes, against `expect`, the rules of lq_sequel.set_scrap / set_subreads and the
device's domain restated here in Python over the (name, tags) a record was written from.  Records are written by tests/bam_writer.py.
Exact comparisons: flags, items, the control throughput, the resume position, the error's code and the record it names."""
import ctypes as C
import struct

import numpy as np
import pytest

from longqc_amd import api, sequel
from tests import bam_writer as BW
from tests import test_launch_caps as LC
from tests.test_polread_walk import model

HDR = BW.header()
ITEM, FLAGGED, CONTROL = 1, 2, 4
VOID = 0x7fffffff
LTILE = LC.header_define("LQ_FXSCAN_LINE_TILE")
SIZES = {"A": 1, "c": 1, "C": 1, "s": 2, "S": 2, "i": 4, "I": 4, "f": 4}


# ---- tags ---------------------------------------------------------------------------------------------------------------------------
def tag(name, ty, value):
    """one aux field: name (2 bytes), type letter, value bytes as they lie in the file"""
    return name + ty.encode() + value


def tag_a(name, letter):
    return tag(name, "A", letter.encode())


def tag_b(name, sub, count, payload=None):
    return tag(name, "B", sub.encode() + struct.pack("<I", count) + (bytes(count * SIZES[sub]) if payload is None else payload))


SN = tag_b(b"sn", "f", 4, struct.pack("<4f", 7.5, 8.25, 9.0, 10.5))
IP = tag_b(b"ip", "C", 5000, bytes(range(250)) * 20)
RG = tag(b"RG", "Z", b"a1b2c3d4\0")
SCALARS = (tag(b"x1", "c", b"\x80") + tag(b"x2", "C", b"\xff") + tag(b"x3", "s", b"sz") + tag(b"x4", "S", b"sc") + tag(b"x5", "i", b"szAN")
           + tag(b"x6", "I", b"scAL") + tag(b"x7", "f", b"\0\0\x80\x3f") + tag(b"x8", "A", b"s"))
HX = tag(b"hx", "H", b"1AE301\0")


def parse_aux(aux):
    """-> {tag: (type, value)} of the first sz and sc, or None if the area is malformed (by the SAM specification's 4.2.4, plus htslib's d)"""
    out, a, n = {}, 0, len(aux)
    while a < n:
        if a + 3 > n:
            return None
        name, ty, v = aux[a:a + 2], chr(aux[a + 2]), a + 3
        if ty in SIZES or ty == "d":
            ln = SIZES.get(ty, 8)
            if ty == "d":
                out["d"] = True                                     # (not a type of the specification: the device leaves the record to the host)
        elif ty in "ZH":
            z = aux.find(b"\0", v)
            if z < 0:
                return None
            ln = z - v + 1
        elif ty == "B":
            if v + 5 > n or chr(aux[v]) not in SIZES or aux[v] == ord("A"):
                return None
            ln = 5 + SIZES[chr(aux[v])] * struct.unpack_from("<I", aux, v + 1)[0]
        else:
            return None
        if v + ln > n:
            return None
        if name in (b"sz", b"sc") and name not in out:
            out[name] = (ty, aux[v:v + ln])
        a = v + ln
    return out


def letter(t):
    """what get_tag's value equals: the letter of an A value or of a one-letter Z value, else None (no letter)"""
    ty, v = t
    return chr(v[0]) if ty == "A" or (ty == "Z" and len(v) == 2) else None


def expect(kind, name, aux):
    """-> (result, in_domain): result ("item", zmw, start, end, class) | ("control", v) | ("none",) | ("error", code); in_domain: the device
    answers itself (a record outside the domain is flagged and the twin gives the result)"""
    in_domain, cls, is_control = True, "S", False
    if kind == 0:
        tags = parse_aux(aux)
        if tags is None:
            return ("error", -2), False
        if b"sz" not in tags or b"sc" not in tags:
            return ("none",), "d" not in tags
        in_domain = tags[b"sz"][0] == "A" and tags[b"sc"][0] == "A" and "d" not in tags
        sz, cls = letter(tags[b"sz"]), letter(tags[b"sc"])
        if sz == "C":
            is_control = True
        elif sz != "N":
            return ("none",), in_domain
    f = name.decode("latin-1").split("/")
    ok = len(f) >= 3 and len(f[2].split("_")) >= 2
    digits = lambda t: t.isascii() and t.isdigit()
    if ok:
        z, (s, e) = f[1], f[2].split("_")[:2]
        ok = all(digits(t) and len(t) <= 9 for t in (z, s, e)) and not (len(z) > 1 and z[0] == "0")
    in_domain = in_domain and ok
    if len(f) < 3:
        return ("error", -2), False
    if is_control and cls != "F":
        return ("none",), in_domain
    pos = f[2].split("_")
    if len(pos) < 2 or not digits(pos[0]) or not digits(pos[1]):
        return ("error", -2), False
    s, e = int(pos[0]), int(pos[1])
    if s > 999999999 or e > 999999999:
        return ("error", -5), False
    if is_control:
        return ("control", e - s + 1), in_domain
    if not (digits(f[1]) and len(f[1]) <= 9 and not (len(f[1]) > 1 and f[1][0] == "0")):
        return ("error", -5), False
    return ("item", int(f[1]), s, e, ord(cls) if cls else 1), in_domain


# ---- the calls ------------------------------------------------------------------------------------------------------------------------
def rec(name, aux=b"", l_seq=3):
    return BW.record(name, b"ACGTN"[:l_seq], None, tags=aux)


def fields(lib, kind, data, start=len(HDR)):
    lib = sequel._lib(lib)
    buf = np.frombuffer(bytes(data), dtype=np.uint8)
    cap = buf.size // 36 + 2
    flags, items = np.zeros(cap, np.uint32), np.zeros((cap, 4), np.uint32)
    n_rows, n_slots, control, resume, err = C.c_uint64(), C.c_uint64(), C.c_int64(), C.c_uint64(), C.create_string_buffer(512)
    rc = lib.lqpol_fields(0, kind, buf.ctypes.data if buf.size else None, buf.size, start, flags.ctypes.data, items.ctypes.data, cap, C.byref(n_rows),
                          C.byref(n_slots), C.byref(control), C.byref(resume), err, 512)
    if rc:
        raise api.LqcovError(rc, err.value.decode())
    return flags[:n_rows.value].tolist(), [tuple(int(x) for x in r) for r in items[:n_slots.value]], control.value, resume.value


def twin(lib, kind, record, rec_no=1):
    lib = sequel._lib(lib)
    item, control, flags, err = (C.c_uint32 * 4)(), C.c_int64(), C.c_uint32(), C.create_string_buffer(768)
    rc = lib.lqpol_twin(kind, record, len(record), rec_no, item, C.byref(control), C.byref(flags), err, 768)
    if rc:
        return ("error", rc), err.value.decode()
    if flags.value == ITEM:
        return ("item",) + tuple(item), ""
    return (("control", control.value) if flags.value == CONTROL else ("none",)), ""


def check_records(lib, kind, recs):
    """recs: [(name, aux)] -> the device's answer, the twin's and the two together against `expect`, record by record"""
    data = HDR + b"".join(rec(n, a) for n, a in recs)
    want = [expect(kind, n, a) for n, a in recs]
    flags, slots, control, resume = fields(lib, kind, data)
    assert resume == len(data) and len(flags) == len(recs)
    k, dev_control = 0, 0
    for i, ((res, dom), f) in enumerate(zip(want, flags)):
        what = (i, recs[i][0], res, dom, f)
        t_res, t_msg = twin(lib, kind, rec(*recs[i]), i + 1)
        assert t_res == res, what + (t_res, t_msg)                   # the twin reads every record, in the domain or not
        if res[0] == "error":
            assert ("record %d '" % (i + 1)).encode() + recs[i][0].split(b"\0")[0] in t_msg.encode("latin-1"), t_msg
        if not dom:
            assert f == FLAGGED and slots[k][0] == VOID, what
            k += 1
            continue
        assert f == {"item": ITEM, "control": CONTROL, "none": 0}[res[0]], what
        if res[0] == "item":
            assert slots[k] == res[1:], what
            k += 1
        elif res[0] == "control":
            dev_control += res[1]
    assert k == len(slots) and control == dev_control
    return want


def run_bytes(lib, scraps, subreads, cut=None):
    """both record lists through lqpol_add_bytes (cut: the scraps bytes arrive in two calls, cut there) -> the finished handle"""
    p = sequel.PolymeraseReads(lib=lib)
    for kind, recs in ((0, scraps), (1, subreads)):
        data = HDR + b"".join(rec(n, a) for n, a in recs)
        if kind == 0 and cut is not None:
            r = p.add_bytes(0, data[:cut], len(HDR))
            assert r <= cut
            assert p.add_bytes(0, data[r:], 0) == len(data) - r
        else:
            assert p.add_bytes(kind, data, len(HDR)) == len(data)
    sequel._finish_lenient(p)
    return p


def by_model(scraps, subreads):
    """{zmw: model(items)} and the control throughput from `expect`, scraps before subreads"""
    items, control = {}, 0
    for kind, recs in ((0, scraps), (1, subreads)):
        for n, a in recs:
            res, _ = expect(kind, n, a)
            assert res[0] != "error"
            if res[0] == "item":
                items.setdefault(res[1], []).append((res[2], res[3], chr(res[4])))
            elif res[0] == "control":
                control += res[1]
    return {z: model(l) for z, l in items.items()}, control


def result(p):
    return {int(z): (int(h), int(t), bool(i), int(a)) for z, h, t, i, a in zip(p.all_zmw, p.all_hq, p.all_tot, p.is_pol, p.all_ad_num)}


NC = tag_a(b"sz", "N")


def check_layouts_and_classes(lib):
    L = lambda c: tag_a(b"sc", c)
    layouts = [NC + L("A"), L("L") + NC, SN + NC + L("F"), NC + SN + L("B"), NC + L("A") + SN, IP + NC + L("L"), NC + IP + L("A") + IP, RG + NC + L("Q"),
               SCALARS + NC + L("A"), NC + SCALARS + L("L"), HX + L("A") + RG + NC + HX, NC + L("A") + NC + L("L") + tag_a(b"sz", "C")]
    recs = [(b"m/%d/%d_%d" % (100 + k, 10 * k, 10 * k + 7), a) for k, a in enumerate(layouts)]
    want = check_records(lib, 0, recs)
    assert all(r[0] == "item" and d for r, d in want)
    assert want[-1][0][4] == ord("A")                               # the first sz and the first sc count
    classes = [(b"m/1/0_10", L("A")), (b"m/1/0_10", NC), (b"m/1/0_10", b""), (b"m/2/5_50", NC + L("A")), (b"m/2/7_900", tag_a(b"sz", "C") + L("F")),
               (b"m/2/900_7", tag_a(b"sz", "C") + L("F")), (b"m/2/7_900", tag_a(b"sz", "C") + L("A")), (b"m/3/1_2", tag_a(b"sz", "X") + L("F")),
               (b"no_slash", tag_a(b"sz", "X") + L("F")), (b"no_slash", L("F")), (b"m/4/0_999999999", tag_a(b"sz", "C") + L("F"))]
    want = check_records(lib, 0, classes)
    assert [r[0] for r, _ in want] == ["none", "none", "none", "item", "control", "control", "none", "none", "none", "none", "control"]
    assert [r[1] for r, _ in want if r[0] == "control"] == [894, -892, 1000000000]
    names = [(b"movie/5/1_2", b""), (b"movie/5/1_2/ccs", b""), (b"a/b/6/1_2", b""), (b"m/7/10_20_30", b""), (b"m/0/0_0", b""), (b"m/999999999/000000007_0999", b""),
             (b"/8/1_2", b""), (b"m/9/1_2_", b"")]
    want = check_records(lib, 1, names)
    assert [r for r, _ in want] == [("item", 5, 1, 2, 83), ("item", 5, 1, 2, 83), ("error", -2), ("item", 7, 10, 20, 83), ("item", 0, 0, 0, 83),
                                    ("item", 999999999, 7, 999, 83), ("item", 8, 1, 2, 83), ("item", 9, 1, 2, 83)]
    assert check_records(lib, 0, [(n, a + NC + tag_a(b"sc", "L")) for n, a in names]) is not None


# (name, aux, kind, what the run must do: an item's class, "none", or the error's code)
FLAGGED_CASES = [
    (b"m/55", b"", 1, -2), (b"m/55", NC + tag_a(b"sc", "A"), 0, -2), (b"m/55", tag_a(b"sz", "C") + tag_a(b"sc", "A"), 0, -2),
    (b"m/55/1x_5", b"", 1, -2), (b"m/55/1_5x", b"", 1, -2), (b"m/55/_5", b"", 1, -2), (b"m/55/15", b"", 1, -2), (b"m/55/ 1_5", b"", 1, -2),
    (b"m/55/1234567890_5", b"", 1, -5), (b"m/55/1_1234567890", NC + tag_a(b"sc", "A"), 0, -5), (b"m/55/0000000012_5", b"", 1, "S"),
    (b"m/007/1_5", b"", 1, -5), (b"m/1234567890/1_5", b"", 1, -5), (b"m/z5/1_5", NC + tag_a(b"sc", "A"), 0, -5),
    (b"m/007/1_5", tag_a(b"sz", "C") + tag_a(b"sc", "F"), 0, "control"),
    (b"m/55/1_5", tag(b"sz", "Z", b"N\0") + tag_a(b"sc", "A"), 0, "A"), (b"m/55/1_5", NC + tag(b"sc", "Z", b"L\0"), 0, "L"),
    (b"m/55/1_5", tag(b"sz", "Z", b"NN\0") + tag_a(b"sc", "A"), 0, "none"), (b"m/55/1_5", tag(b"sz", "C", b"N") + tag_a(b"sc", "A"), 0, "none"),
    (b"m/55/1_5", NC + tag(b"sc", "i", b"A\0\0\0"), 0, "\x01"),
    (b"m/55/1_5", NC + tag_a(b"sc", "A") + tag(b"ip", "B", b"C" + struct.pack("<I", 9) + bytes(8)), 0, -2),
    (b"m/55/1_5", tag(b"ip", "B", b"C" + struct.pack("<I", 0xffffffff)) + NC + tag_a(b"sc", "A"), 0, -2),
    (b"m/55/1_5", NC + tag_a(b"sc", "A") + tag(b"qq", "?", b"\0"), 0, -2), (b"m/55/1_5", NC + tag_a(b"sc", "A") + b"xy", 0, -2),
    (b"m/55/1_5", NC + tag_a(b"sc", "A") + tag(b"RG", "Z", b"open"), 0, -2), (b"m/55/1_5", tag(b"dd", "d", bytes(8)) + NC + tag_a(b"sc", "A"), 0, "A"),
    (b"m/55/1_5", tag(b"ba", "B", b"A" + struct.pack("<I", 1) + b"x") + NC + tag_a(b"sc", "A"), 0, -2),
]


def check_flagged(lib):
    for name, aux, kind, outcome in FLAGGED_CASES:
        good = [(b"m/55/5_9", NC + tag_a(b"sc", "L") if kind == 0 else b""), (b"m/56/0_4", NC + tag_a(b"sc", "A") if kind == 0 else b"")]
        recs = [good[0], (name, aux), good[1]]
        want = check_records(lib, kind, recs)
        assert not want[1][1], (name, aux)                            # outside the domain: the device flags it
        scraps, subreads = (recs, [(b"m/56/4_9", b"")]) if kind == 0 else ([(b"m/56/9_9", NC + tag_a(b"sc", "A"))], recs)
        if isinstance(outcome, int):
            with pytest.raises(api.LqcovError) as e:
                run_bytes(lib, scraps, subreads)
            assert e.value.code == outcome and ("%s record 2 '%s'" % (("scraps", "subreads")[kind], name.decode())) in str(e.value), str(e.value)
            continue
        assert want[1][0][0] == ("item" if len(outcome) == 1 else outcome) and (len(outcome) != 1 or want[1][0][4] == ord(outcome))
        p = run_bytes(lib, scraps, subreads)
        m, control = by_model(scraps, subreads)
        assert result(p) == m and p.control_throughput == control
        assert p.stats["records_flagged"] == 1 and p.stats["records_device"] == 3 and p.stats["records_host"] == 0


def check_order_through_the_twin(lib):
    """a flagged record keeps its place among the items: ties at equal (start, end) on both sides of it"""
    z = tag(b"sz", "Z", b"N\0")
    for classes in ("LAF", "ALF", "AFL", "FLA"):
        scraps = [(b"m/9/40_90", (z if k == 1 else NC) + tag_a(b"sc", c)) for k, c in enumerate(classes)] + [(b"m/9/0_40", NC + tag_a(b"sc", "A"))]
        subreads = [(b"m/9/90_200", b""), (b"m/9/40_90", b"")]
        p = run_bytes(lib, scraps, subreads)
        assert result(p) == by_model(scraps, subreads)[0] and p.stats["records_flagged"] == 1
    assert len({tuple(by_model([(b"m/9/40_90", NC + tag_a(b"sc", c)) for c in cl], [(b"m/9/0_40", b"")])[0][9]) for cl in ("LA", "AL")}) == 2


def check_layout(lib):
    rng = np.random.default_rng(9)
    scraps = [(b"m/%d/%d_%d" % (rng.integers(1, 40), s, s + rng.integers(0, 90)), (IP if k % 50 == 7 else b"") + NC + tag_a(b"sc", "ALFB"[k % 4]))
              for k, s in enumerate(rng.integers(0, 5000, 2 * LTILE + 1).tolist())]
    subreads = [(b"m/%d/%d_%d" % (rng.integers(1, 40), s, s + rng.integers(0, 900)), b"") for s in rng.integers(0, 5000, 300).tolist()]
    m, control = by_model(scraps, subreads)
    data = HDR + b"".join(rec(n, a) for n, a in scraps)
    ends = np.cumsum([len(HDR)] + [len(rec(n, a)) for n, a in scraps]).tolist()
    # records at one block - 1, one block, one block + 1: the device's flags and slots
    for n in (LTILE - 1, LTILE, LTILE + 1):
        flags, slots, _, resume = fields(lib, 0, data[:ends[n]])
        assert flags == [ITEM] * n and resume == ends[n]
        assert slots == [expect(0, *r)[0][1:] for r in scraps[:n]]
    # a record that straddles the end of the bytes given: cut inside its fixed fields, its name, its tags, and at a record boundary
    for cut in (ends[100] + 20, ends[100] + 40, ends[101] - 1, ends[57], ends[57] + 5011):
        flags, slots, _, resume = fields(lib, 0, data[:cut])
        assert resume == max(e for e in ends if e <= cut) and len(flags) == ends.index(resume)
        p = run_bytes(lib, scraps, subreads, cut=cut)
        assert result(p) == m and p.control_throughput == control
    # records the device walk does not vouch for (aligned: refID 0) are the host's, in their place
    mixed = list(scraps[:40])
    parts = [HDR]
    for k, (n, a) in enumerate(mixed):
        r = bytearray(rec(n, a))
        if k in (0, 7, 8, 9, 39):
            r[4:8] = struct.pack("<i", 0)
        parts.append(bytes(r))
    p = sequel.PolymeraseReads(lib=lib)
    assert p.add_bytes(0, b"".join(parts), len(HDR)) == sum(len(x) for x in parts)
    assert p.add_bytes(1, HDR + rec(b"m/1/0_5"), len(HDR)) == len(HDR) + len(rec(b"m/1/0_5"))
    sequel._finish_lenient(p)
    assert result(p) == by_model(mixed, [(b"m/1/0_5", b"")])[0]
    assert 5 <= p.stats["records_host"] <= 8 and p.stats["records_host"] + p.stats["records_device"] == 41      # (between two scans the host may take a record more)
    # the order of the files is enforced
    p = sequel.PolymeraseReads(lib=lib)
    p.add_bytes(1, HDR + rec(b"m/1/0_5"), len(HDR))
    with pytest.raises(api.LqcovError) as e:
        p.add_bytes(0, HDR + rec(b"m/1/0_5", NC + tag_a(b"sc", "A")), len(HDR))
    assert e.value.code == -4 and "scraps after subreads" in str(e.value)


def random_record(rng):
    """-> (kind, name, aux): mostly well-formed, with every kind of damage now and then"""
    kind = int(rng.integers(0, 2))
    num = lambda: str(int(rng.integers(0, 10 ** int(rng.integers(1, 10)))))
    z, s, e = num(), num(), num()
    r = rng.random()
    if r < 0.04:
        z = "0" + z
    elif r < 0.08:
        s = "0" * int(rng.integers(1, 12)) + s
    elif r < 0.12:
        e = e + str(rng.integers(0, 10 ** 3))
    elif r < 0.15:
        s = s[:1] + "x+ _"[int(rng.integers(0, 4))] + s[1:]
    name = "/".join((["mv"] * int(rng.integers(0, 3)) + [z, s + "_" + e] + ["t"] * int(rng.integers(0, 2)))[:int(rng.integers(1, 6))])
    if rng.random() < 0.03:
        name = name.replace("_", "", 1)
    pool = [SN, RG, HX, SCALARS, tag_b(b"pw", "S", int(rng.integers(0, 40))), tag(b"dd", "d", bytes(8))]
    tags = [pool[int(i)] for i in rng.integers(0, len(pool), int(rng.integers(0, 4)))]
    for nm in (b"sz", b"sc"):
        r = rng.random()
        if r < 0.8:
            tags.append(tag_a(nm, ("NNNCCCX" if nm == b"sz" else "FFFALSB")[int(rng.integers(0, 7))]))
        elif r < 0.86:
            tags.append(tag(nm, "Z", [b"N\0", b"C\0", b"F\0", b"NN\0", b"\0"][int(rng.integers(0, 5))]))
        elif r < 0.9:
            tags.append(tag(nm, "C", b"N"))
    tags = [tags[int(i)] for i in rng.permutation(len(tags))]
    aux = b"".join(tags)
    r = rng.random()
    if r < 0.04 and aux:
        aux = aux[:-int(rng.integers(1, min(len(aux), 6) + 1))]
    elif r < 0.07:
        aux += [b"x", b"xy", tag(b"zz", "?", b"1"), tag(b"bb", "B", b"q" + struct.pack("<I", 1)), tag(b"bb", "B", b"i" + struct.pack("<I", 1 << 30))][int(rng.integers(0, 5))]
    return kind, name.encode(), aux


def check_twin(lib, n=3000, every_outcome=True):
    rng = np.random.default_rng(21)
    recs = [random_record(rng) for _ in range(n)]
    seen = {}
    for kind in (0, 1):
        mine = [(nm, a) for k, nm, a in recs if k == kind]
        for (res, dom) in check_records(lib, kind, mine):
            seen[(res[0] if res[0] != "error" else res, dom)] = seen.get((res[0] if res[0] != "error" else res, dom), 0) + 1
    # every outcome occurs on both sides of the domain's border
    for key in () if not every_outcome else (("item", True), ("item", False), ("control", True), ("control", False), ("none", True), ("none", False), (("error", -2), False), (("error", -5), False)):
        assert seen.get(key, 0) >= 3, (key, seen)


CHECKS = [check_layouts_and_classes, check_flagged, check_order_through_the_twin, check_layout, check_twin]


@pytest.mark.parametrize("check", CHECKS, ids=lambda f: f.__name__)
def test_emulated_fields(emu_lib, check):
    check(emu_lib)


@pytest.mark.parametrize("order", LC.ORDERS[1:])
def test_emulated_fields_in_other_thread_orders(emu_lib, monkeypatch, order):
    LC.set_order(monkeypatch, order)
    check_layout(emu_lib)
    check_twin(emu_lib, n=600, every_outcome=False)


@pytest.mark.gpu
@pytest.mark.parametrize("check", CHECKS, ids=lambda f: f.__name__)
def test_gpu_fields(gpu_lib, check):
    check(gpu_lib)
