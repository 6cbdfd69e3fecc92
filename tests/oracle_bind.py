"""Test-side access to the checker (oracle/): the CPU restatement and, where present, the compiled
reference (oracle/_ref).  Imported only by tests/, __graft_entry__.smoke() and bench.py's
cpu_baseline leg -- never by longqc_amd/.

ref_table / ref_dump / ref_sdust / ref_index run the reference's binaries where oracle/_ref is built; elsewhere the
output the reference printed (and the file it wrote) for the same argv and the same input bytes, recorded under
tests/golden/ref_runs/ (LQCOV_RECORD_REF=1 records while the binaries run: tests/golden/make_ref_runs.py), stands in."""
import gzip
import hashlib
import os
import subprocess
from typing import List, Optional, Sequence

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORACLE_DIR = os.path.join(ROOT, "oracle")
ORACLE_CLI = os.path.join(ORACLE_DIR, "lqcov_oracle")
REF_BIN = os.path.join(ORACLE_DIR, "_ref", "minimap2-coverage")
REF_HARNESS = os.path.join(ORACLE_DIR, "_ref", "ref_harness")
REF_SDUST = os.path.join(ORACLE_DIR, "_ref", "sdust")
RECORDED = os.path.join(ROOT, "tests", "golden", "ref_runs")


def ensure_oracle():
    if not os.path.exists(ORACLE_CLI):
        subprocess.run(["make", "-C", ORACLE_DIR, "oracle"], check=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    return ORACLE_CLI


def have_ref() -> bool:
    return os.path.exists(REF_BIN) and os.path.exists(REF_HARNESS)


def table(argv: List[str], extra: Optional[List[str]] = None) -> str:
    """9-column table of the CPU restatement for a minimap2-coverage argv."""
    ensure_oracle()
    r = subprocess.run([ORACLE_CLI, "table"] + (extra or []) + [str(a) for a in argv], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    if r.returncode != 0:
        raise RuntimeError("oracle failed: " + r.stderr[-2000:])
    return r.stdout


def dump(what: str, opts: List[str], files: List[str]) -> str:
    ensure_oracle()
    r = subprocess.run([ORACLE_CLI, what] + opts + files, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    if r.returncode != 0:
        raise RuntimeError("oracle failed: " + r.stderr[-2000:])
    return r.stdout


def _run_key(tool: str, args: Sequence[str], outputs: Sequence[str]) -> str:
    """a run is its binary, its argv and the bytes of the files it reads (temporary paths differ from run to run, contents do not)"""
    h = hashlib.sha256(tool.encode())
    for a in args:
        if a in outputs:
            h.update(b"\0out")
        elif os.path.isfile(a):
            with open(a, "rb") as f:
                h.update(b"\0file" + hashlib.sha256(f.read()).digest())
        else:
            h.update(b"\0arg" + a.encode())
    return h.hexdigest()[:32]


def _save_gz(path: str, data: bytes):
    with open(path, "wb") as f, gzip.GzipFile(fileobj=f, mode="wb", mtime=0) as g:
        g.write(data)


def _ref_run(tool: str, exe: str, args: Sequence, outputs: Sequence[str] = ()) -> str:
    """stdout of the reference's `tool` (its files in `outputs` written); RuntimeError if it fails"""
    args = [str(a) for a in args]
    key = _run_key(tool, args, outputs)
    fn = os.path.join(RECORDED, key + ".gz")
    r = subprocess.run([exe] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE) if os.path.exists(exe) else None
    if r is not None and r.returncode == 2 and r.stderr.startswith(b"usage:") and os.path.exists(fn):
        r = None                                                # a harness built before this command existed: the recorded run stands in
    if r is not None:
        if r.returncode != 0:
            raise RuntimeError("%s failed (%d): %s" % (tool, r.returncode, r.stderr.decode(errors="replace")[-2000:]))
        if os.environ.get("LQCOV_RECORD_REF") == "1":
            os.makedirs(RECORDED, exist_ok=True)
            _save_gz(os.path.join(RECORDED, key + ".gz"), r.stdout)
            for i, o in enumerate(outputs):
                with open(o, "rb") as f:
                    _save_gz(os.path.join(RECORDED, "%s.out%d.gz" % (key, i)), f.read())
        return r.stdout.decode()
    if not os.path.exists(fn):
        raise RuntimeError("%s: oracle/_ref is not built and no run of the reference with these inputs is recorded "
                           "(tests/golden/make_ref_runs.py records them where it is)" % tool)
    for i, o in enumerate(outputs):
        with gzip.open(os.path.join(RECORDED, "%s.out%d.gz" % (key, i)), "rb") as f, open(o, "wb") as g:
            g.write(f.read())
    with gzip.open(fn, "rb") as f:
        return f.read().decode()


def ref_table(argv: List[str]) -> str:
    """9-column table of the reference's minimap2-coverage for an argv."""
    return _ref_run("minimap2-coverage", REF_BIN, argv)


def ref_index(argv: List[str], out: str) -> str:
    """the reference's minimap2-coverage with `-d out` in argv: writes the index file `out`"""
    return _ref_run("minimap2-coverage", REF_BIN, argv, outputs=[out])


def ref_dump(args: List[str]) -> str:
    return _ref_run("ref_harness", REF_HARNESS, args)


def ref_sdust(args: List[str]) -> str:
    """table of the reference's second binary, sdust"""
    return _ref_run("sdust", REF_SDUST, args)
