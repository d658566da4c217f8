"""The host side of sampling (sli.h: sli_sample, sli_model_set_sampling and its getters): the symbols, and every
SLI_ERR_ARG refusal of the op, each decided before the device is touched. No call here would pass the checks, so the
pointers are never followed."""
import ctypes
import math

import pytest

from simplellminference_amd import _lib, ops  # (ops imports torch ahead of libsli.so, as the GPU files do)
from simplellminference_amd.model import LlamaModel

ERR_ARG = 1
FAKE = ctypes.c_void_p(0x1000)  # non-null, never dereferenced


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def test_symbols_exist(lib):
    for name in ("sli_sample", "sli_model_set_sampling", "sli_model_get_sampling", "sli_model_get_sampled",
                 "sli_model_graph_captures"):
        assert hasattr(lib, name) and name in _lib.exported_symbols()
    assert callable(ops.sample)
    for name in ("set_sampling", "sampling", "sampled", "graph_captures"):
        assert callable(getattr(LlamaModel, name))
    assert ctypes.sizeof(_lib.Sampling) == 16
    assert [f[0] for f in _lib.Sampling._fields_] == ["temperature", "top_k", "top_p", "seed"]


def _sample(lib, prm, logits=FAKE, row_stride=1000, rows=4, vocab=1000, pos=FAKE, pos_stride=1, out=FAKE):
    p = ctypes.byref(_lib.Sampling(*prm)) if prm is not None else None
    rc = lib.sli_sample(logits, row_stride, rows, vocab, p, 0, pos, pos_stride, out, None)
    return rc, lib.sli_last_error().decode()


@pytest.mark.parametrize("t", [0.0, -1.0, math.nan, 0.0099, 100.5, math.inf, -math.inf])
def test_temperature_out_of_range(lib, t):
    rc, msg = _sample(lib, (t, 0, 1.0, 0))
    assert rc == ERR_ARG and "temperature" in msg


@pytest.mark.parametrize("p", [0.0, -0.5, 1.0000001, 2.0, math.nan, math.inf])
def test_top_p_out_of_range(lib, p):
    rc, msg = _sample(lib, (1.0, 0, p, 0))
    assert rc == ERR_ARG and "top_p" in msg


@pytest.mark.parametrize("k", [-1, -(2 ** 31)])
def test_top_k_negative(lib, k):
    rc, msg = _sample(lib, (1.0, k, 1.0, 0))
    assert rc == ERR_ARG and "top_k" in msg


@pytest.mark.parametrize("which", ["logits", "pos", "out", "prm"])
def test_null_pointers(lib, which):
    kw = {which: None} if which != "prm" else {}
    rc, msg = _sample(lib, None if which == "prm" else (1.0, 0, 1.0, 0), **kw)
    assert rc == ERR_ARG and "null" in msg


@pytest.mark.parametrize("kw", [dict(rows=0), dict(rows=-3), dict(vocab=0), dict(vocab=-1),
                                dict(row_stride=999), dict(row_stride=-1000), dict(pos_stride=-1)])
def test_shape_arguments(lib, kw):
    rc, msg = _sample(lib, (1.0, 0, 1.0, 0), **kw)
    assert rc == ERR_ARG and "sli_sample" in msg


def test_model_entry_points_refuse_null(lib):
    v = ctypes.c_int32()
    prm = _lib.Sampling(1.0, 0, 1.0, 0)
    assert lib.sli_model_set_sampling(None, ctypes.byref(prm)) == ERR_ARG
    assert lib.sli_model_get_sampling(None, ctypes.byref(prm)) == ERR_ARG
    assert lib.sli_model_get_sampled(None, 0, ctypes.byref(v)) == ERR_ARG
    assert lib.sli_model_graph_captures(None, ctypes.byref(v)) == ERR_ARG
