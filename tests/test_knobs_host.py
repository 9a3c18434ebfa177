"""KNOBS.md lists every LAV_* environment variable that the sources read, and nothing else."""
import glob
import os
import re

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _names(files, pattern):
    found = set()
    for f in files:
        with open(f, errors="replace") as fh:
            found.update(re.findall(pattern, fh.read()))
    return found


def test_knobs_table_matches_the_sources():
    """Both directions: a variable that the C++ or the Python sources quote must have a row, and a row must be read somewhere.  On
    the C++ side every string literal that is exactly a LAV_* name counts, wherever it stands: a name handed to a helper that calls
    getenv() for it is read as much as one inside getenv(...).  A quoted name ending in '_' is a family prefix
    (os.environ.get("LAV_TRAIN_" + what)): at least one row carries it, and it justifies the rows that do."""
    py = (glob.glob(os.path.join(REPO, "lav_amd", "**", "*.py"), recursive=True) + glob.glob(os.path.join(REPO, "*.py"))
          + glob.glob(os.path.join(REPO, "tests", "golden", "make_golden*.py")))
    assert os.path.join(REPO, "bench.py") in py
    read = _names(glob.glob(os.path.join(REPO, "lav_amd", "csrc", "*")), r'"(LAV_[A-Z0-9_]+)"')
    assert len(read) > 20 and "LAV_CONV_SPLIT" in read, "the C++ sources were not found"
    read |= _names(py, r'''["'](LAV_[A-Z0-9_]+)["']''')
    families = {n for n in read if n.endswith("_")}
    read -= families
    with open(os.path.join(REPO, "KNOBS.md")) as fh:
        tables = [re.findall(r"^\| `(LAV_[A-Z0-9_]+)` \|", part, re.M) for part in fh.read().split("\n## ")]
    assert all(t == sorted(t) for t in tables), "the rows of a table are sorted by name"
    rows = sum(tables, [])
    assert rows and len(rows) == len(set(rows)), "a variable has two rows"
    missing = sorted(read - set(rows)) + sorted(f + "*" for f in families if not any(r.startswith(f) for r in rows))
    stale = sorted(r for r in set(rows) - read if not any(r.startswith(f) for f in families))
    assert not missing, f"read by the sources, no row in KNOBS.md: {missing}"
    assert not stale, f"rows of KNOBS.md that nothing reads: {stale}"
