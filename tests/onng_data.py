"""The onng2k fixtures (tests/golden/make_onng_goldens.py) for the ONNG tests."""
import functools
import gzip
import os
import shutil
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
ONNG2K = os.path.join(GOLD, "onng2k")
sys.path.insert(0, GOLD)
import ngt_files as F  # noqa: E402

# name -> (outgoing, incoming, path adjustment, min edges, input fixture)
CASES = {
    "onng_s": (5, 40, False, 0, "anng"),
    "onng_S": (5, 40, True, 0, "anng"),
    "onng_E": (5, 40, True, 12, "anng"),
    "onng_P": (0, 0, True, 0, "anng"),
    "onng_R": (30, 40, False, 0, "onng_S"),
    "onng_R2": (8, 20, True, 0, "onng_S"),
}


def anng_grp_bytes():
    with gzip.open(os.path.join(ONNG2K, "anng", "grp.gz"), "rb") as f:
        return f.read()


def make_anng_dir(dst):
    """The input ANNG index directory (grp unpacked) at `dst`."""
    os.makedirs(dst)
    for f in ("obj", "prf", "tre"):
        shutil.copy(os.path.join(ONNG2K, "anng", f), os.path.join(dst, f))
    with open(os.path.join(dst, "grp"), "wb") as f:
        f.write(anng_grp_bytes())
    return dst


@functools.lru_cache(maxsize=None)
def csr(name):
    """(offsets, ids, dists) of a fixture graph; shared, do not modify."""
    if name == "anng":
        import tempfile
        with tempfile.TemporaryDirectory() as t:
            p = os.path.join(t, "grp")
            with open(p, "wb") as f:
                f.write(anng_grp_bytes())
            g = F.read_grp(p)
    else:
        g = F.read_grp(os.path.join(ONNG2K, name, "grp"))
    for a in g:
        a.setflags(write=False)
    return g
