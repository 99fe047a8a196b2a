"""The copy-edit-run runner that tools/scan_mutants.py, tools/stats_mutants.py, tools/cut_mutants.py and tools/partial_mutants.py share.  CPU only, not part of the test run.

A mutant is (name, what it does, [(file, search text, replacement, number of sites)]).  run_mutant copies the tree's sources to a
temporary directory, applies the edits there (each search text must occur in its file exactly as often as the entry says: a stale
entry fails loudly), runs ONE test file in the copy -- the emulator library builds itself from the mutated sources -- and reports:
survived, or killed and by what (a failed assertion, a crash of the emulator, a time-out) and in which test first."""
import argparse
import concurrent.futures
import os
import shutil
import subprocess
import sys
import tempfile
import xml.etree.ElementTree as ET

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TIMEOUT = 900
NEEDED = ("fastplong_amd", "tests", "oracle", "include")  # what the emulator tests read: the sources, not what was built from them
SKIP = shutil.ignore_patterns("__pycache__", ".pytest_cache", "_ref", "*.so", "*.o", "*.tmp.*")


def run_mutant(entry, tests, select=()):
    """tests: the test file, relative to the root; select: further pytest arguments (-k EXPR) -> (name, what, stopped by, first test)"""
    name, what, edits = entry
    with tempfile.TemporaryDirectory(prefix="mutant_%s_" % name) as tmp:
        tree = os.path.join(tmp, "tree")
        for d in NEEDED:
            shutil.copytree(os.path.join(ROOT, d), os.path.join(tree, d), ignore=SKIP, symlinks=True)
        for rel in dict.fromkeys(e[0] for e in edits):
            path = os.path.join(tree, rel)
            with open(path) as f:
                text = f.read()
            for _, search, repl, sites in (e for e in edits if e[0] == rel):
                found = text.count(search)
                assert found == sites, "%s: %r occurs %d times in %s, not %d: the entry is stale" % (name, search, found, rel, sites)
                text = text.replace(search, repl)
            with open(path, "w") as f:
                f.write(text)
        env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1")
        report = os.path.join(tmp, "report.xml")
        try:
            p = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-p", "no:cacheprovider", "--junitxml=" + report, tests, *select],
                               cwd=tree, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=TIMEOUT)
        except subprocess.TimeoutExpired:
            return name, what, "time-out", ""
        if p.returncode == 0:
            return name, what, "SURVIVED", ""
        if p.returncode < 0 or p.returncode > 128 or not os.path.exists(report):
            return name, what, "crash (status %d)" % p.returncode, ""
        # the first test that did not pass, and whether an assertion stopped it (not, say, a header that no longer compiles)
        for case in ET.parse(report).getroot().iter("testcase"):
            for kind in ("failure", "error"):
                f = case.find(kind)
                if f is not None:
                    msg = f.get("message") or ""
                    how = "assertion" if kind == "failure" and msg.startswith("AssertionError") else "error: " + msg[:80]
                    return name, what, how, case.get("name")
        return name, what, "error (status %d)" % p.returncode, ""


def arguments(tests):
    ap = argparse.ArgumentParser()
    ap.add_argument("-j", "--jobs", type=int, default=max(1, min(8, (os.cpu_count() or 2) // 2)))
    ap.add_argument("--only", nargs="*")
    ap.add_argument("--markdown", action="store_true")
    ap.add_argument("-k", dest="select", help="run only the tests of %s that match (pytest -k)" % tests)
    return ap


def run_table(mutants, tests, a):
    """run the entries a.only names (all when none), print the table -> the names of those an assertion did NOT stop"""
    todo = [m for m in mutants if not a.only or m[0] in a.only]
    select = ["-k", a.select] if a.select else []
    with concurrent.futures.ThreadPoolExecutor(a.jobs) as ex:
        rows = list(ex.map(lambda m: run_mutant(m, tests, select), todo))
    if a.markdown:
        print("| mutant | what it breaks | stopped by | first test that fails |\n|---|---|---|---|")
        for name, what, how, test in rows:
            print("| `%s` | %s | %s | `%s` |" % (name, what, how, test))
    else:
        for name, what, how, test in rows:
            print("%-13s %-28s %s" % (name, how, test))
    bad = [r[0] for r in rows if r[2] != "assertion"]
    print("%d mutants, %d killed by an assertion%s" % (len(rows), len(rows) - len(bad), "; NOT: " + " ".join(bad) if bad else ""))
    return bad
