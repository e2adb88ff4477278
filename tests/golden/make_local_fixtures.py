"""Pack the larger third-party test data into tests/golden/<set>/ (run once, in a checkout of the reference sources).

Sets (what the tests read; tests/local_data.py writes them out into tests/_local_data/<set>/):
  rm1     the RM1 decode task: the CD-continuous 8-Gaussian RM1 model of sphinx4's models, its dictionary and filler
          dictionary, sphinx3's RM 2845-sentence trigram LM (DMP), and the cepstra of the first 20 utterances of
          SphinxTrain's rm1_train.fileids.100 with their control file rm.ctl
  ps      pocketsphinx's hub4wsj_sc_8k (US English) and tdt_sc_8k (Mandarin) semi-continuous models, the Mandarin
          5000-word trigram LM and dictionary, and three of its test recordings (goforward, numbers, something .raw)
  ps_ptm  pocketsphinx-extra's US-English PTM model hub4_wsj_ptm256_3s_8k.cd_ptm_5000 and pocketsphinx's goforward.fsg

Every file is stored xz-compressed; a compressed file larger than PART bytes is cut into numbered parts, so that no
committed file reaches 1 MiB.  MANIFEST.json holds each file's parts, size and SHA-256.  The data is mostly float model
parameters that do not compress: the sets are what the tests need, not small.

    python tests/golden/make_local_fixtures.py <reference checkout> [set ...]
"""
import hashlib
import json
import lzma
import os
import shutil
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
PART = 1000000
N_RM_UTT = 20


def sources(ref, name):
    """-> {file name in the set: bytes}"""
    rd = lambda *p: open(os.path.join(ref, *p), "rb").read()
    out = {}
    if name == "rm1":
        rm = os.path.join("sphinx4", "models", "acoustic", "rm1")
        out["mdef"] = rd(rm, "etc", "RM1_clean_13dCep_16k_40mel_130Hz_6800Hz.1800.mdef")
        for f in ("fillerdict", "RM.dictionary"):
            out[f] = rd(rm, "dict", f)
        for f in ("means", "variances", "mixture_weights", "transition_matrices"):
            out[f] = rd(rm, "cd_continuous_8gau", f)
        out["RM.2845.trigram.arpa.DMP"] = rd("sphinx3", "src", "tests", "performance", "rm1", "RM.2845.trigram.arpa.DMP")
        feat = os.path.join("SphinxTrain", "test", "res", "feat", "rm")
        utts = [l.split()[0] for l in rd(feat, "rm1_train.fileids.100").decode().splitlines() if l.strip()][:N_RM_UTT]
        out["rm.ctl"] = "".join(u + "\n" for u in utts).encode()
        for u in utts:
            out[f"feat/{u}.mfc"] = rd(feat, u + ".mfc")
    elif name == "ps":
        for model, d in (("hub4wsj_sc_8k", ("en_US", "hub4wsj_sc_8k")), ("tdt_sc_8k", ("zh", "tdt_sc_8k"))):
            src = os.path.join("pocketsphinx", "model", "hmm", *d)
            for f in sorted(os.listdir(os.path.join(ref, src))):
                out[f"{model}/{f}"] = rd(src, f)
        for f in ("gigatdt.5000.DMP", "mandarin_notone.dic"):
            out[f"zh_CN/{f}"] = rd("pocketsphinx", "model", "lm", "zh_CN", f)
        for u in ("goforward", "numbers", "something"):
            out[f"raw/{u}.raw"] = rd("pocketsphinx", "test", "data", u + ".raw")
    elif name == "ps_ptm":
        src = os.path.join("pocketsphinx-extra", "model", "hmm", "en_US", "hub4_wsj_ptm256_3s_8k.cd_ptm_5000")
        for f in sorted(os.listdir(os.path.join(ref, src))):
            out[f"hub4_wsj_ptm256_3s_8k.cd_ptm_5000/{f}"] = rd(src, f)
        out["goforward.fsg"] = rd("pocketsphinx", "test", "data", "goforward.fsg")
    else:
        raise SystemExit(f"unknown set {name}")
    return out


def pack(ref, name):
    dst = os.path.join(HERE, name)
    shutil.rmtree(dst, ignore_errors=True)
    os.makedirs(dst)
    manifest = {}
    for f, raw in sorted(sources(ref, name).items()):
        z = lzma.compress(raw, preset=9 | lzma.PRESET_EXTREME)
        stored = f.replace("/", "__") + ".xz"
        chunks = [z[i:i + PART] for i in range(0, len(z), PART)]
        parts = [stored] if len(chunks) == 1 else [f"{stored}.{k:02d}" for k in range(len(chunks))]
        for p, c in zip(parts, chunks):
            with open(os.path.join(dst, p), "wb") as fh:
                fh.write(c)
        manifest[f] = {"parts": parts, "size": len(raw), "sha256": hashlib.sha256(raw).hexdigest()}
    with open(os.path.join(dst, "MANIFEST.json"), "w") as fh:
        json.dump(manifest, fh, indent=1, sort_keys=True)
        fh.write("\n")


if __name__ == "__main__":
    for s in sys.argv[2:] or ("rm1", "ps", "ps_ptm"):
        pack(sys.argv[1], s)
