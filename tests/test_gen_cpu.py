"""The host side of per-sequence generation (sli.h: sli_sample_gen, sli_model_set_gen_seq and its getters): the
symbols, the struct's layout, and every SLI_ERR_ARG refusal of the op, each decided before the device is touched. No
call here would pass the checks, so the pointers are never followed."""
import ctypes
import math

import pytest

from simplellminference_amd import _lib, ops  # (ops imports torch ahead of libsli.so, as the GPU files do)
from simplellminference_amd.model import LlamaModel

ERR_ARG = 1
FAKE = ctypes.c_void_p(0x1000)  # non-null, never dereferenced
OK = dict(temperature=1.0, top_k=0, top_p=1.0, seed=0, min_p=0.0, repetition_penalty=1.0, presence_penalty=0.0,
          frequency_penalty=0.0, penalty_from=0, max_pos=0)


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def test_symbols_exist(lib):
    for name in ("sli_sample_gen", "sli_model_set_gen_seq", "sli_model_get_gen_seq", "sli_model_get_finished"):
        assert hasattr(lib, name) and name in _lib.exported_symbols()
    assert callable(ops.sample_gen) and callable(ops.gen_params)
    for name in ("set_generation", "generation", "finished", "generate"):
        assert callable(getattr(LlamaModel, name))


def test_struct_layout():
    G = _lib.GenParams
    assert [f[0] for f in G._fields_] == ["temperature", "top_k", "top_p", "seed", "min_p", "repetition_penalty",
                                          "presence_penalty", "frequency_penalty", "penalty_from", "max_pos", "n_stop",
                                          "stop"]
    assert ctypes.sizeof(G) == 4 * 11 + 4 * 8 == 76 and _lib.MAX_STOP == 8
    assert [getattr(G, n).offset for n, _ in G._fields_] == [4 * i for i in range(12)]
    assert ctypes.sizeof(_lib.Sampling) == 16  # sli_sampling is what it was
    p = ops.gen_params(0.5, 3, 0.9, 2 ** 32 + 7, 0.1, 1.2, 0.3, 0.4, 5, 9, stop=(11, 12))
    assert (p.seed, p.penalty_from, p.max_pos, p.n_stop, list(p.stop)[:3]) == (7, 5, 9, 2, [11, 12, 0])


def _gen(lib, rows=2, bad_row=1, hist=FAKE, hist_stride=16, logits=FAKE, pos=FAKE, out=FAKE, row_stride=1000,
         vocab=1000, pos_stride=1, prm=True, **kw):
    blocks = (_lib.GenParams * max(rows, 1))(*[ops.gen_params(**(dict(OK, **kw) if r == bad_row else OK))
                                              for r in range(max(rows, 1))])
    rc = lib.sli_sample_gen(logits, row_stride, rows, vocab, blocks if prm else None, 0, pos, pos_stride, hist,
                            hist_stride, out, None)
    return rc, lib.sli_last_error().decode()


@pytest.mark.parametrize("field,value", [
    ("temperature", -1.0), ("temperature", math.nan), ("temperature", 0.0099), ("temperature", 100.5),
    ("temperature", math.inf), ("temperature", 1e-30),
    ("top_k", -1), ("top_k", -(2 ** 31)),
    ("top_p", 0.0), ("top_p", -0.5), ("top_p", 1.0000001), ("top_p", math.nan),
    ("min_p", -1e-6), ("min_p", 1.0), ("min_p", 2.0), ("min_p", math.nan),
    ("repetition_penalty", 0.0999), ("repetition_penalty", 10.001), ("repetition_penalty", math.nan),
    ("repetition_penalty", -1.0),
    ("presence_penalty", -100.01), ("presence_penalty", 100.01), ("presence_penalty", math.nan),
    ("frequency_penalty", -100.01), ("frequency_penalty", 100.01), ("frequency_penalty", math.nan),
    ("penalty_from", -1), ("max_pos", -1)])
def test_block_out_of_range(lib, field, value):
    rc, msg = _gen(lib, **{field: value})
    assert rc == ERR_ARG and field in msg and "row 1" in msg


@pytest.mark.parametrize("n", [-1, 9])
def test_n_stop_out_of_range(lib, n):
    blocks = (_lib.GenParams * 1)(ops.gen_params(**OK))
    blocks[0].n_stop = n
    rc = lib.sli_sample_gen(FAKE, 1000, 1, 1000, blocks, 0, FAKE, 1, FAKE, 16, FAKE, None)
    assert rc == ERR_ARG and "n_stop" in lib.sli_last_error().decode()


@pytest.mark.parametrize("kw", [dict(repetition_penalty=1.1), dict(presence_penalty=0.1), dict(frequency_penalty=-0.1)])
def test_null_history_with_an_active_penalty(lib, kw):
    rc, msg = _gen(lib, hist=None, **kw)
    assert rc == ERR_ARG and "hist_dev" in msg
    rc, msg = _gen(lib, hist_stride=0, **kw)
    assert rc == ERR_ARG and "hist_stride" in msg


@pytest.mark.parametrize("which", ["logits", "pos", "out", "prm"])
def test_null_pointers(lib, which):
    rc, msg = _gen(lib, **({which: None} if which != "prm" else {"prm": False}))
    assert rc == ERR_ARG and "null" in msg


@pytest.mark.parametrize("kw", [dict(rows=0), dict(rows=-3), dict(vocab=0), dict(vocab=-1), dict(row_stride=999),
                                dict(row_stride=-1000), dict(pos_stride=-1)])
def test_shape_arguments(lib, kw):
    rc, msg = _gen(lib, **kw)
    assert rc == ERR_ARG and "sli_sample_gen" in msg


def test_model_entry_points_refuse_null(lib):
    v = (ctypes.c_int32 * 8)()
    prm = ops.gen_params(**OK)
    assert lib.sli_model_set_gen_seq(None, 0, ctypes.byref(prm)) == ERR_ARG
    assert lib.sli_model_get_gen_seq(None, 0, ctypes.byref(prm)) == ERR_ARG
    assert lib.sli_model_get_finished(None, v) == ERR_ARG
