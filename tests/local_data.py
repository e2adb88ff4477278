"""The larger third-party test data (tests/golden/make_local_fixtures.py): the RM1 decode task ("rm1"), pocketsphinx's
semi-continuous models, Mandarin LM and recordings ("ps"), and its US-English PTM model ("ps_ptm").

Each set is committed compressed under tests/golden/<set>/ (MANIFEST.json: parts, size and SHA-256 of every file).
path(set) writes the set out into tests/_local_data/<set>/ (git-ignored), where the reference decoders and the drop-in
programs read it, checks every file there against the manifest, and returns the directory.  Call it inside a test or
fixture: a damaged fixture then fails the tests that need it."""
import hashlib
import json
import lzma
import os

from conftest import GOLDEN, ROOT

OUT = os.path.join(ROOT, "tests", "_local_data")
_done = set()


def _same(path, ent):
    if not os.path.isfile(path) or os.path.getsize(path) != ent["size"]:
        return False
    with open(path, "rb") as f:
        return hashlib.sha256(f.read()).hexdigest() == ent["sha256"]


def path(name):
    """-> tests/_local_data/<name>, its files written out from tests/golden/<name>/ where missing or different"""
    dst_dir = os.path.join(OUT, name)
    if name in _done:
        return dst_dir
    src = os.path.join(GOLDEN, name)
    with open(os.path.join(src, "MANIFEST.json")) as f:
        manifest = json.load(f)
    for fname, ent in sorted(manifest.items()):
        dst = os.path.join(dst_dir, fname)
        if _same(dst, ent):
            continue
        raw = lzma.decompress(b"".join(open(os.path.join(src, p), "rb").read() for p in ent["parts"]))
        assert len(raw) == ent["size"] and hashlib.sha256(raw).hexdigest() == ent["sha256"], f"tests/golden/{name}: {fname} is damaged"
        os.makedirs(os.path.dirname(dst), exist_ok=True)
        tmp = f"{dst}.tmp{os.getpid()}"
        with open(tmp, "wb") as f:
            f.write(raw)
        os.replace(tmp, dst)            # (atomic: a concurrent reader sees the old file or the whole new one)
    _done.add(name)
    return dst_dir
