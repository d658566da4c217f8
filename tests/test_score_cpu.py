"""The host side of scoring (sli.h: sli_score_rows, sli_model_score_seqs, sli_model_score_seqs_ok): the symbols, and
every argument refusal, each decided before the device is touched. No call here would pass the checks, so the pointers
are never followed. The model-level argument checks are one host routine shared with sli_model_prefill_seqs; a model
cannot exist without a device, so they are reached through the test hook sli_debug_prefill_seqs_args, which runs that
routine for given model dimensions (their order is sli_model_prefill_seqs's: tests/test_gpu_batch_prefill.py)."""
import ctypes

import numpy as np
import pytest

from simplellminference_amd import _lib, ops  # (ops imports torch ahead of libsli.so, as the GPU files do)
from simplellminference_amd.model import LlamaModel

ERR_ARG, ERR_RANGE = 1, 3
FAKE = ctypes.c_void_p(0x1000)  # non-null, 16-byte aligned, never dereferenced


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def test_symbols_exist(lib):
    for name in ("sli_score_rows", "sli_model_score_seqs", "sli_model_score_seqs_ok"):
        assert hasattr(lib, name) and name in _lib.exported_symbols()
    header = open(_lib.LIB_PATH.rsplit("/", 2)[0] + "/include/sli.h").read()
    for name in ("sli_score_rows(", "sli_model_score_seqs(", "sli_model_score_seqs_ok("):
        assert "int " + name in header
    assert callable(ops.score_rows) and callable(ops.prefill_gemm_logits) and ops.PF_ROLE_LOGITS == 3
    for name in ("score_ok", "score", "perplexity"):
        assert callable(getattr(LlamaModel, name))


def _rows(lib, logits=FAKE, M=4, V=1000, ld=1000, targets=FAKE, logprob=FAKE, top=None, tlp=None):
    rc = lib.sli_score_rows(logits, M, V, ld, targets, logprob, top, tlp, None)
    return rc, lib.sli_last_error().decode()


@pytest.mark.parametrize("which", ["logits", "targets", "logprob"])
def test_score_rows_null_pointers(lib, which):
    rc, msg = _rows(lib, **{which: None})
    assert rc == ERR_ARG and "null" in msg


@pytest.mark.parametrize("kw", [dict(M=0), dict(M=-2), dict(V=0), dict(V=-1), dict(ld=999), dict(ld=996),
                                dict(V=17, ld=17), dict(V=17, ld=18), dict(ld=1002),
                                dict(logits=ctypes.c_void_p(0x1004))])
def test_score_rows_shape_arguments(lib, kw):
    rc, msg = _rows(lib, **kw)
    assert rc == ERR_ARG and "sli_score_rows" in msg


def test_model_entry_points_refuse_null(lib):
    a = (ctypes.c_int32 * 4)()
    f = (ctypes.c_float * 4)()
    assert lib.sli_model_score_seqs_ok(None) == 0
    for args in ((None, a, 1, a, a, 4, f), (FAKE, None, 1, a, a, 4, f), (FAKE, a, 1, None, a, 4, f),
                 (FAKE, a, 1, a, None, 4, f), (FAKE, a, 1, a, a, 4, None)):
        assert lib.sli_model_score_seqs(*args, None, None) == ERR_ARG
        assert "null" in lib.sli_last_error().decode()


def _args(lib, seqs, prompts, batch=4, max_len=64, vocab=512, n_seqs=None):
    ld = max(1, max(len(p) for p in prompts))
    P = np.zeros((len(prompts), ld), np.int32)
    for i, p in enumerate(prompts):
        P[i, :len(p)] = p
    lens = np.array([len(p) for p in prompts], np.int32)
    s = np.array(seqs, np.int32)
    rc = lib.sli_debug_prefill_seqs_args(batch, max_len, vocab, s.ctypes.data_as(ctypes.c_void_p),
                                         len(seqs) if n_seqs is None else n_seqs, P.ctypes.data_as(ctypes.c_void_p),
                                         lens.ctypes.data_as(ctypes.c_void_p), ld)
    return rc, lib.sli_last_error().decode()


def test_model_argument_refusals(lib):
    assert _args(lib, [0, 1], [[1, 2], [3]])[0] == 0
    assert _args(lib, [0], [[1, 2]], n_seqs=0) == (ERR_ARG, "prefill_seqs: n_seqs must be in [1, batch]")
    assert _args(lib, [0, 1, 2, 3, 0], [[1]] * 5)[0] == ERR_ARG  # n_seqs above the batch
    assert _args(lib, [4], [[1, 2]])[1] == "prefill_seqs: sequence index out of range"
    assert _args(lib, [-1], [[1, 2]])[0] == ERR_ARG
    assert _args(lib, [1, 1], [[1, 2], [3, 4]]) == (ERR_ARG, "prefill_seqs: a sequence is listed twice")
    assert _args(lib, [0, 1], [[1, 2], []]) == (ERR_RANGE, "prompt length out of range")
    assert _args(lib, [0], [[1] * 65])[0] == ERR_RANGE  # longer than the context
    assert _args(lib, [0], [[1, 512]]) == (ERR_RANGE, "Token index is greater than vocab size.")
    assert _args(lib, [0], [[1, -1]])[0] == ERR_RANGE


def test_model_argument_refusals_come_in_prefill_seqs_order(lib):
    """sli_model_prefill_seqs: the count, then per sequence its index and its duplicates, then per prompt its length
    and its tokens; a call wrong in several ways reports the earliest."""
    bad_tok, bad_len = [1, 999], []
    assert "n_seqs" in _args(lib, [9, 9], [bad_tok, bad_len], n_seqs=5)[1]
    assert "out of range" in _args(lib, [9, 9], [bad_tok, bad_len])[1] and _args(lib, [9, 9], [bad_tok, bad_len])[0] == ERR_ARG
    assert "listed twice" in _args(lib, [1, 1], [bad_tok, bad_len])[1]
    assert "Token index" in _args(lib, [0, 1], [bad_tok, bad_len])[1]  # prompt 0's token before prompt 1's length
    assert "length" in _args(lib, [0, 1], [bad_len, bad_tok])[1]
    assert "listed twice" in _args(lib, [2, 2, 7], [[1], [1], [1]])[1]  # sequence 1's duplicate before sequence 2's index
