"""The block entry points of the multi-stream scorer (s3a_ms_mgau_score_frames[_dev], s3a_ms_mgau_set_block_chunk)
as far as they go without a GPU: exported, bound, declared, and refusing a NULL handle before any HIP call."""
import ctypes as C
import os
import re

import numpy as np

from conftest import ROOT
from cmusphinx_amd import lib

NAMES = ("s3a_ms_mgau_score_frames", "s3a_ms_mgau_score_frames_dev", "s3a_ms_mgau_set_block_chunk")
S3A_EINVAL = -1


def test_symbols_are_exported_and_bound():
    L = lib.load()
    for n in NAMES:
        assert n in lib._SIGS, n
        assert n not in lib.MISSING and hasattr(L, n), n


def test_null_handle_is_einval_without_a_device():
    L = lib.load()
    feat = np.zeros((2, 4), np.float32)
    scr = np.zeros((2, 3), np.int32)
    best = np.zeros(2, np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert L.s3a_ms_mgau_score_frames(None, p(feat), 2, None, p(scr), p(best), 0) == S3A_EINVAL
    assert L.s3a_ms_mgau_score_frames_dev(None, p(feat), 4, 2, None, p(scr), 3, p(best), 0, None) == S3A_EINVAL
    assert L.s3a_ms_mgau_set_block_chunk(None, 5) == S3A_EINVAL
    assert not scr.any() and not best.any()


def test_raw_flag_in_the_header_is_one():
    src = open(os.path.join(ROOT, "include", "cmusphinx_amd.h")).read()
    m = re.search(r"^#define\s+S3A_MS_RAW\s+(\S+)", src, flags=re.M)
    assert m and int(m.group(1), 0) == 1
    assert lib.MS_RAW == 1
