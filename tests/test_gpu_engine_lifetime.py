"""An engine's whole life, several times in one process (MI355X): init, the second pass enabled, lattices kept, a queue of 7 ragged tidigits
utterances through 3 lanes, everything read, free -- three times over, then a plain decode on a fourth engine.  Every buffer of an engine is
allocated through one owner and freed by it (s3a_hostmem.h), and the buffers of a call grow on demand; what comes out must not depend on
which life of which engine decoded it.  3 lanes and 7 utterances: as launches the lanes are refilled at window boundaries; through
ku_frames (S3A_UTT_PERSIST) the queue is groups of 3, 3 and 1.

Expected values are the ones test_gpu_queue.py and test_gpu_dag.py already hold: the unmodified reference's -hyp / -hypseg lines, and the
second pass's words and lattice sizes recorded from the reference's own tables (tests/golden/dag_tables.npz, case "tidigits")."""
import os

import numpy as np
import pytest

from cmusphinx_amd import bundle
from conftest import GOLDEN
from test_gpu_queue import ref_lines, tidigits_feats
from test_gpu_uttdec import tidigits_bundle  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu
N_UTT, N_LANES = 7, 3


def golden_second_pass(k):
    """(words [n, 5] = wid sf ef ascr lscr, lattice nodes, lattice links) of tidigits utterance k"""
    G = np.load(os.path.join(GOLDEN, "dag_tables.npz"))
    hdr = G[f"tidigits.{k}.hdr"]
    assert int(hdr[4]) >= 0
    return np.stack([G[f"tidigits.{k}.o_{key}"] for key in ("wid", "sf", "ef", "ascr", "lscr")], axis=1), int(hdr[5]), int(hdr[6])


@pytest.mark.parametrize("persist", [None, "1"])
def test_engines_come_and_go_and_decode_the_same(gpu_lib, tidigits_bundle, monkeypatch, persist):
    if persist is not None:
        monkeypatch.setenv("S3A_UTT_PERSIST", persist)
    utts, feats = tidigits_feats(gpu_lib)
    rm, rs = ref_lines()
    want = [golden_second_pass(k) for k in range(N_UTT)]
    assert len({len(f) for f in feats[:N_UTT]}) == N_UTT         # ragged
    seen = []
    for cycle in range(3):
        dec = bundle.Decoder(tidigits_bundle, N_LANES, bestpath=True)
        dec.ud.queue_keep_lattices()
        dec.decode_queue(feats[:N_UTT])
        assert dec.ud.last_parts()["n_frames"] == (3 if persist else 0)         # (ku_frames: one launch chain per group of 3, 3 and 1)
        got = []
        for u in range(N_UTT):
            hdr, words = dec.queue_hyp(u, utts[u][1], u)
            assert hdr.status == 0, (cycle, u, hdr.status)
            lines = dec.format_var(hdr, words)
            h2, w2 = dec.queue_bestpath_hyp(u, utts[u][1], u)
            info, nodes, links = dec.ud.queue_lattice(u)
            print(f"cycle {cycle} utterance {u}: second pass status {h2.status}, {h2.n_words} words; lattice {info.n_nodes} nodes / "
                  f"{info.n_links} links (golden {want[u][1]} / {want[u][2]})")
            assert lines == (rm[u], rs[u]), (cycle, u)
            assert h2.status == 0 and np.array_equal(np.asarray(w2)[:, :5], want[u][0]), (cycle, u)
            assert (info.n_nodes, info.n_links) == want[u][1:], (cycle, u)
            assert len(nodes) == info.n_nodes and len(links) == info.n_links
            got.append((lines, bytes(h2), np.asarray(w2).tobytes(), bytes(np.asarray(nodes)), bytes(np.asarray(links))))
        seen.append(got)
        dec.ud.__del__()                # s3a_uttdec_free now, not when the collector gets to it
    assert seen[1] == seen[0] and seen[2] == seen[0]
    # a fourth engine, lock step: lane z = utterance z
    dec = bundle.Decoder(tidigits_bundle, N_LANES, bestpath=True)
    dec.decode(feats[:N_LANES])
    assert dec.ud.last_parts()["n_frames"] == (1 if persist else 0)
    for z in range(N_LANES):
        assert dec.format_var(*dec.hyp_var(z, utts[z][1], z)) == (rm[z], rs[z]), z
        h2, w2 = dec.bestpath_hyp(z, utts[z][1], z)
        info, nodes, links = dec.ud.lattice(z)
        assert h2.status == 0 and np.array_equal(np.asarray(w2)[:, :5], want[z][0]), z
        assert (info.n_nodes, info.n_links) == want[z][1:], z
        assert bytes(np.asarray(nodes)) == seen[0][z][3] and bytes(np.asarray(links)) == seen[0][z][4], z
    dec.ud.__del__()
