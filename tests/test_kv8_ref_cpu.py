"""tests/kv8_ref.py against torch's float8_e4m3fn and against the rule of include/sli.h itself (CPU only).

torch rounds 464 (the midpoint of 448 and the NaN code's would-be value 480) to 448 and turns everything above it
into NaN, so torch is the second opinion only for |x| <= 464; past it the rule (saturate to +-448) is stated alone.
"""
import numpy as np
import pytest
import torch

from tests import kv8_ref as K


def f8_inputs():
    """Every code value, every midpoint between adjacent codes, the midpoints +- 1 fp32 ulp, the subnormal range on
    a fine grid, +-0; both signs."""
    mags = K.MAGS.astype(np.float32)
    mids = K.MIDS.astype(np.float32)
    assert np.array_equal(mids.astype(np.float64), K.MIDS)  # the midpoints are fp32 numbers
    up = np.nextafter(mids, np.float32(np.inf))
    dn = np.nextafter(mids, np.float32(-np.inf))
    sub = np.arange(0, 8 * 64 + 1, dtype=np.float32) * np.float32(2.0 ** -15)  # 0 .. 2^-6 in steps of 2^-15
    tiny = np.array([2.0 ** -10, 2.0 ** -11, 1e-30, 1e-40], np.float32)
    tiny = np.concatenate([tiny, np.nextafter(tiny[:1], np.float32(1)), np.nextafter(tiny[:1], np.float32(0))])
    pos = np.concatenate([mags, mids, up, dn, sub, tiny])
    return np.concatenate([pos, -pos]).astype(np.float32)


def test_decode_is_torchs_table():
    codes = np.arange(256, dtype=np.uint8)
    want = torch.from_numpy(codes).view(torch.float8_e4m3fn).float().numpy()
    got = K.decode(codes)
    nan = (codes & 0x7F) == 0x7F
    assert np.array_equal(np.isnan(got), nan) and np.array_equal(np.isnan(want), nan)
    assert np.array_equal(got[~nan].view(np.uint32), want[~nan].view(np.uint32))  # 254 codes, -0 included
    assert got[0x7E] == 448 and got[0x01] == 2.0 ** -9 and got[0x08] == 2.0 ** -6 and got[0x38] == 1.0
    # exact in fp16
    assert np.array_equal(got[~nan].astype(np.float16).astype(np.float32), got[~nan])


def test_encode_is_torchs_rounding_up_to_464():
    x = f8_inputs()
    x = x[np.abs(x) <= 464]
    want = torch.from_numpy(x).to(torch.float8_e4m3fn).view(torch.uint8).numpy()
    assert np.array_equal(K.encode(x), want)
    edge = np.array([448, np.nextafter(np.float32(448), np.float32(500)), 464, -464], np.float32)
    assert np.array_equal(torch.from_numpy(edge).to(torch.float8_e4m3fn).view(torch.uint8).numpy(),
                          [0x7E, 0x7E, 0x7E, 0xFE])
    assert np.isnan(torch.tensor([465.0]).to(torch.float8_e4m3fn).float().numpy()[0])  # why torch stops at 464


def test_encode_round_trips_and_ties_to_even():
    codes = np.array([c for c in range(256) if (c & 0x7F) != 0x7F], np.uint8)
    assert np.array_equal(K.encode(K.decode(codes)), codes)  # -0 -> 0x80 among them
    for c in range(0x7E):
        mid = np.float32(K.MIDS[c])
        assert K.encode(mid) == (c if c % 2 == 0 else c + 1)
        assert K.encode(np.nextafter(mid, np.float32(0))) == c
        assert K.encode(np.nextafter(mid, np.float32(1e9))) == c + 1


def test_saturation_and_nan_follow_the_rule():
    big = np.array([448, 449, 464, 465, 480, 1e9, 3e38, np.inf], np.float32)
    assert np.all(K.encode(big) == 0x7E) and np.all(K.encode(-big) == 0xFE)
    assert K.encode(np.float32(np.nan)) == 0x7F and K.encode(-np.float32(np.nan)) == 0x7F
    assert K.encode(np.float32(0.0)) == 0x00 and K.encode(np.float32(-0.0)) == 0x80
    assert K.encode(np.float32(2.0 ** -10)) == 0x00  # the tie between 0 and 2^-9 goes to the even code
    assert K.encode(np.nextafter(np.float32(2.0 ** -10), np.float32(1))) == 0x01
    # float64 input (the restatement's unrounded values) follows the same boundaries
    assert K.encode(np.float64(K.MIDS[5]) * (1 + 1e-15)) == 6 and K.encode(np.float64(K.MIDS[5]) * (1 - 1e-15)) == 5


# ---------------------------------------------------------------- the reference alone
PROMPTS = [[1, 17, 42, 99], [5, 6], [300, 2, 77, 8, 9], [11]]  # the ragged prompts of test_gpu_batch.py
PROMPTS8 = PROMPTS + [[7, 3, 250], [64, 65, 66, 67, 68, 69], [2], [123, 45]]
# (preset, weights, seed, prompts, positions): the runs of tests/test_gpu_kv8.py's model tests; the seeds are
# test_gpu_batch_i8.py's (tiny 4, tiny-gqa 11, small-h128-gqa 3, tiny-h8 4) and test_gpu_mxfp4.py's (tiny-gqa 1)
MODEL_RUNS = [("tiny", "f16", 4, PROMPTS[:1], 36), ("tiny", "i8", 4, PROMPTS[:1], 36),
              ("tiny-gqa", "f16", 11, PROMPTS, 36), ("tiny-gqa", "i8", 11, PROMPTS, 36),
              ("tiny-gqa", "mxfp4", 1, PROMPTS[:1], 36), ("small-h128-gqa", "i8", 3, PROMPTS8, 24),
              ("tiny-h8", "i8", 4, PROMPTS, 36)]


@pytest.mark.parametrize("name,w_dtype,seed,prompts,n", MODEL_RUNS)
def test_reference_alone_fp32_against_float64(oracle, name, w_dtype, seed, prompts, n):
    """The condition the GPU model test rests on, without a GPU: an fp32-numpy copy of the restatement walks against
    the float64 one through the same helper, with the slack measured the same way (4 x the largest K/V row difference
    of the two UNROUNDED runs). Its adopted flips must stay under a quarter of the cap, and its logits meet the bar.
    No seed needed replacing: every run here has zero or a handful of flips (printed)."""
    from simplellminference_amd.model import preset
    cfg = preset(name)
    oc, W = K.weights(oracle, cfg, seed, w_dtype)
    for b, prompt in enumerate(prompts):
        toks = K.pad_prompt(prompt, n, cfg.vocab_size, b)
        rows64, _ = K.unrounded_rows(oc, W, toks)
        rows32, _ = K.unrounded_rows(oc, W, toks, dtype=np.float32)
        slack = K.slack_from(rows64, lambda l, p, which: rows32[p][l][which])
        m32 = K.Model8(oc, W, dtype=np.float32)
        codes, logits32 = {}, []

        def adopt(l, p, which, unrounded, own):
            codes[(l, p, which)] = own
            return own
        for p, t in enumerate(toks):
            logits32.append(m32.forward(int(t), p, adopt=adopt))
        logits64, w = K.walk_run(oc, W, toks, lambda l, p, which: codes[(l, p, which)], slack)
        K.check_flips(w, f"{name} {w_dtype} seq {b}", cap=K.FLIP_CAP / 4)
        K.check_logits(np.array(logits32), logits64, f"{name} {w_dtype} seq {b}")
