"""The decode attention (simplellminference_amd/csrc/attention.h, attn_mfma.h, attn_mfma_f8.h) one launch at a time,
through the kernel-level entry of sli.h (sli_decode_attn, "decode stages, for tests and labs"), against the float64
reference tests/attn_ref.py (itself held to the C oracle by test_attn_ref_cpu.py). The entry calls mha_launch with the
engine's own arguments, so it launches the engine's code objects with the engine's batching (seq_heads, strided device
positions, a different position per sequence) and its three merges, on geometries made as if the chip had `cus` compute
units: attn_ref.CELLS are caches of at most 2176 rows whose plans have the geometry class of every production launch
(test_attn_stage_cpu.py holds that cover).

Harness: out and part are filled with NaN sentinels before every launch; the cache is three layers of memory with the
middle one under test; the positions live in an int32 array of stride 6 with poison between the entries; rows past
pos[b] hold poison (+-65504, +-3e38, FP8 +-448; NaN and the FP8 NaN codes in test_nan_past_pos); every launch runs
twice and must be bit-identical; after each launch the arrival counters are all zero.

Cells (attn_ref._cells): R1 register-staged, batch 1, merge 1, fp16 / fp32, hd 128 / 64, G 1 / 2, four splits; R2
register-staged fp16 GQA-4 on both sides of the two-GQA-2-groups condition, and GQA-8; R3 fp32 cache, a batch of 4,
the merge launch, G 1 .. 8, one cell of 17 splits; R4 fp32 cache, batch 1, the in-launch merge against the merge
launch; M1 / M2 the MFMA kernel over fp16 / FP8, a batch of 4, every (hd, G, ring depth) instantiation at 1, 2 and 3
tiles per wave; M3 the entry against ops.mha_strided.

Bars (derivations in attn_ref.py next to each builder and bound):
  (a) needle: one key row scores 4096 / sqrt(hd) >= 362 and every other 0, so every other weight is expf(<= -362) = 0
      exactly: out equals V[t*] BIT FOR BIT, for t* over row 0, pos, and the first and last row of a wave slice, a
      32-key tile and a split (every class in every cell, asserted by the builder); merge 1: the live partials merge
      (gemv_ref.merge) to the same bits.
  (b) uniform: K = 0, so l = pos + 1 and o = sum V, integers: out within 1 fp32 ulp of the float64 quotient, bit for bit
      where pos + 1 is a power of two; every live partial has l = its live row count, o = the integer sum, m = 0.
  (c) realistic: normal q, K, V (rounded to the cache type); on every other head q is scaled by 8 and split 0 lies
      >= 120 below the maximum. Unscaled heads at test_mha's bar (rtol 1e-5, atol 2e-6), scaled heads within
      attn_ref.real_tol; every live partial in its o / l, m + log l form within the same bound of its split.
  (d) nothing else is written: dead splits and pad words of part, part beyond [B hq][max_splits], out when merge 1
      took effect, out beyond B hq hd, the neighbouring layers and the cache, q and the position array.
  (e) cus = the device's count equals cus = 0, bit for bit; merge 0 equals merge 2 bit for bit on the register-staged
      kernel (both merge in split order); the entry equals ops.mha_strided bit for bit.

Measured on an MI355X (27 tests, 8.8 s): every cell of (a) and (b) is bit-exact as stated, with NaN (FP8: the NaN
codes) past pos too (no kernel reads a row past pos: both clamp the row index, so the contract of sli.h allows anything
there); (d) and (e) hold.
(c), the largest error / bound per cell class (scaled heads against attn_ref.real_tol; unscaled heads against rtol
1e-5 + atol 2e-6; the partials' m + log l against real_tol's second result):
            scaled   unscaled   m + log l
      R1    0.008     0.030      0.013
      R2    0.009     0.052      0.019
      R3    0.010     0.104      0.017
      R4    0.009     0.051      0.017
      M1    0.020     0.279      0.030
      M2    0.024     0.191      0.031
      M3    0.010     0.037      0.026
real_tol is worst-case in sqrt(hd) and in the largest |q| |k| of a weighted row, so a correct kernel sits a factor 40 -
100 inside it; what bites on arithmetic is (a) and (b), and (c) guards the realistic ranges (an overflowing expf, a
dropped scale). Nothing was found wrong in the kernels. The R4 pairs run at cus 63, below 2 Hkv wg_splits = 64: at 64
the merge launch's GQA-4 cell would run as two GQA-2 groups, whose partials differ from the unsplit in-launch kernel's
in their wave merge; the test asserts the same geometry on both sides.

That it bites (scratch builds of ops.hip with one arithmetic-only change to a copy of attention.h / attn_mfma.h each,
never out of bounds, not committed; this file run once per build; tests failing of 26, and the bar that caught it first):
  1 attn_pos reads sequence 0 for every kv head     11  (a) needle R3 / M1 / M2: every batched cell returns the row of
                                                        another position; (b), (c), NaN past pos, cus; batch 1 passes
  2 the row clamp at t_end - 2 (MFMA: pos - 1)      22  (a) needle of every cell: the needle at pos is never loaded
  3 the scale dropped                                7  (c) realistic of every cell (the needle and the uniform family
                                                        do not see a scale: 4096 > 362 either way, and 0 is 0)
  4 ch = kvh modulo the kv heads under kv_group 2    6  (a) needle R2 / R3: the second GQA-2 group reads the next head
  5 one more split in attn_live_splits               7  (a) needle R3 / R4: the merge consumes a dead split's sentinel
                                                        (NaN); merge 0 against merge 2, cus; merge 1 and MFMA do not use it
  6 the merge's M taken from split 0                11  (a) needle R3 / R4 / M1 / M2 / M3: with the needle in a later
                                                        split expf overflows; (c) where split 0 lies 120 below
  7 the partial's l is wave 0's, not the merged L   22  (a) needle of every cell; (b) l is not the live row count
  8 a wave whose first row is pos counted dead      10  (a) needle R1 .. R4 (of 27 tests, with the positions below): pos
    (live_wave = t0 < pos, attention.h)                 = 0, a slice, ppwg on the fp16 and the fp32 geometry; (b) the same
Every cell runs every listed position (0, a slice minus 1 and a slice, 31, 32, ppwg - 1, ppwg, the odd one in the last
split, T - 1): a batch in each family, a batch-1 cell over its needle and uniform launches together
(attn_ref.cell_sets; test_attn_stage_cpu.py asserts it).
"""
import zlib

import numpy as np
import pytest

from tests import attn_ref as R
from tests import gemv_ref as G
from tests.test_gpu_prefill_kernels import _hold, _is_sentinel, _sentinel

pytestmark = pytest.mark.gpu

PAD = 7  # sentinel elements behind out and part
RATIOS = {}
NAMES = ("R1", "R2", "R3", "R4", "M1", "M2", "M3")


def _seed(c, fam, i):
    return zlib.crc32(f"{R.cell_id(c)}|{fam}|{i}".encode()) & 0x7FFFFFFF


def _ratio(key, err, tol):
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(tol > 0, err / tol, 0.0)
    if r.size:
        RATIOS[key] = max(RATIOS.get(key, 0.0), float(np.nanmax(r)))


def _finish(fails):
    assert not fails, f"{len(fails)} failures:\n" + "\n".join(fails[:25])


def _bits_equal(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


class Launch:
    """The device side of one cell: buffers, the launch (twice), and the checks every family shares."""

    def __init__(self, torch, c, cus=None):
        from simplellminference_amd import _lib, ops
        self.torch, self.c, self.ops = torch, c, ops
        self.cus = c["cus"] if cus is None else cus
        self.B, self.hq, self.hkv, self.hd, self.T, self.kv = c["B"], c["hq"], c["hkv"], c["hd"], c["T"], c["kv"]
        self.H, self.n = self.B * self.hq, self.B * self.hq * self.hd
        self.plan = ops.decode_attn_plan(R.DT[self.kv], self.B, self.hq, self.hkv, self.hd, self.T, merge=c["merge"],
                                         cus=self.cus)
        self.part_floats = _lib.load().sli_mha_workspace_bytes(self.T, self.H, self.hd) // 4 - self.H
        self.used = self.H * self.plan["max_splits"] * (self.hd + 4)
        assert self.used <= self.part_floats  # (the launcher refuses what would not fit; asserted all the same)

    def load(self, q, Kc, Vc, pos):
        torch = self.torch
        assert all(0 <= int(p) < self.T for p in pos) and Kc.shape == (self.B * self.hkv, self.T, self.hd)
        self.pos = [int(p) for p in pos]
        fill = 0x7B if self.kv == "f8" else np.array(-777.0, Kc.dtype)  # the neighbouring layers
        self.K3 = np.full((3,) + Kc.shape, fill, Kc.dtype)
        self.V3 = np.full((3,) + Vc.shape, fill, Vc.dtype)
        self.K3[1], self.V3[1] = Kc, Vc
        self.q, self.pa = np.ascontiguousarray(q, np.float32), R.pos_array(pos)
        self.kd, self.vd = torch.from_numpy(self.K3).cuda(), torch.from_numpy(self.V3).cuda()
        self.qd, self.pd = torch.from_numpy(self.q).cuda(), torch.from_numpy(self.pa).cuda()
        self.cd = torch.zeros(2 * self.B * self.hkv + PAD, dtype=torch.int32, device="cuda")

    def run(self):
        torch = self.torch
        out = _sentinel(torch, (self.n + PAD,), False)
        part = _sentinel(torch, (self.part_floats + PAD,), False)
        plan = self.ops.decode_attn(self.qd, self.kd[1], self.vd[1], out, part, self.cd, self.pd, self.hq,
                                    merge=self.c["merge"], pos_seq_stride=R.POS_STRIDE,
                                    kv_dtype="f8" if self.kv == "f8" else None, cus=self.cus)
        return dict(out=out.cpu().numpy(), part=part.cpu().numpy(), counters=self.cd.cpu().numpy(), plan=plan)

    def twice(self, fails, tag):
        a, b = self.run(), self.run()
        for k in ("out", "part"):
            if not _bits_equal(a[k], b[k]):
                fails.append(f"{tag}: {k} differs between two launches")
        for r in (a, b):
            if r["counters"].any():
                fails.append(f"{tag}: counters not zero after the launch: {np.flatnonzero(r['counters'])[:8].tolist()}")
        if a["plan"] != self.plan:
            fails.append(f"{tag}: the launch ran {a['plan']}, the plan said {self.plan}")
        self.written(fails, tag, a)
        return a

    def ns(self):
        return R.ns_of_heads(self.pos, self.hq, self.plan)

    def parts(self, r):
        return r["part"][:self.used].reshape(self.H, self.plan["max_splits"], self.hd + 4)

    def written(self, fails, tag, r):
        """(d): what must be written is, and nothing else."""
        sent_o, sent_p = _is_sentinel(r["out"]), _is_sentinel(r["part"])
        if not sent_o[self.n:].all():
            fails.append(f"{tag}: out written past B hq hd")
        if self.plan["merge"] == 1:
            if not sent_o.all():
                fails.append(f"{tag}: out written although the merge is the consumer's")
        elif sent_o[:self.n].any():
            fails.append(f"{tag}: {int(sent_o[:self.n].sum())} elements of out not written")
        if not sent_p[self.used:].all():
            fails.append(f"{tag}: part written beyond [B hq][max_splits]")
        sp = sent_p[:self.used].reshape(self.H, self.plan["max_splits"], self.hd + 4)
        live = np.arange(self.plan["max_splits"])[None, :] < self.ns()[:, None]
        if not sp[~live].all():
            fails.append(f"{tag}: a dead split of part was written")
        if not sp[:, :, self.hd + 2:].all():
            fails.append(f"{tag}: a pad word of part was written")
        if sp[live][:, :self.hd + 2].any():
            fails.append(f"{tag}: a live split of part was not written")
        for name, dev, host in (("k", self.kd, self.K3), ("v", self.vd, self.V3), ("q", self.qd, self.q),
                                ("pos", self.pd, self.pa)):
            if not _bits_equal(dev.cpu().numpy(), host):
                fails.append(f"{tag}: {name} was changed")


def _cells(name):
    return [c for c in R.CELLS if c["name"] == name]


def _sets(L, c, fam):
    return R.cell_sets(c, L.plan, fam)


def _live(X, pos, hkv):
    """The values with the rows past pos zeroed: the reference never multiplies the poison (0 * inf)."""
    X = X.copy()
    for kvh in range(X.shape[0]):
        X[kvh, pos[kvh // hkv] + 1:] = 0
    return X


def _merged(L, r):
    """The live partials merged by gemv_ref.merge (float64), as the consumer would: [H hd]."""
    p = L.parts(r).astype(np.float64)
    dead = np.arange(L.plan["max_splits"])[None, :] >= L.ns()[:, None]
    p[dead] = 0.0  # (the sentinels of the dead splits alone: a NaN in a live split stays one)
    return R.merge_heads(p, L.ns(), L.hd)


# ---------------------------------------------------------------- (a) needle
def _needle(torch, c, fails, nan=False):
    L = Launch(torch, c)
    hits = {}
    for i, pos in enumerate(_sets(L, c, "needle")):
        tag = f"{R.cell_id(c)} needle pos {pos}"
        q, Kc, Vc, want = R.needle(pos, L.hq, L.hkv, L.hd, L.T, L.kv, L.plan, _seed(c, "needle", i), hits)
        if nan:
            R.poison_rows(Kc, Vc, pos, L.hkv, L.kv, nan=True)
        L.load(q, Kc, Vc, pos)
        r = L.twice(fails, tag)
        got = _merged(L, r).astype(np.float32) if L.plan["merge"] == 1 else r["out"][:L.n]
        if not _bits_equal(got, want):
            bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
            fails.append(f"{tag}: {bad.size} of {want.size} outputs are not V[t*], first at head {bad[0] // L.hd} "
                         f"dim {bad[0] % L.hd}: {got[bad[0]]} for {want[bad[0]]}")
    assert set(hits) == set(R.NEEDLE_CLASSES), (R.cell_id(c), hits)


@pytest.mark.parametrize("name", NAMES)
def test_needle(gpu, name):
    fails = []
    for c in _cells(name):
        _needle(gpu, c, fails)
    _finish(fails)


def test_nan_past_pos(gpu):
    """The rows past pos[b] hold NaN (an FP8 cache: the NaN codes 0x7F / 0xFF) instead of finite poison, on R1 (fp16 and
    fp32), M1 and M2 cells: no kernel reads them (the register-staged kernel clamps its row index to pos, the MFMA
    kernel's DMA too)."""
    fails = []
    cells = [c for c in R.CELLS if c.get("nan")]
    assert {(c["name"], c["kv"]) for c in cells} == {("R1", "f16"), ("R1", "f32"), ("M1", "f16"), ("M2", "f8")}
    for c in cells:
        _needle(gpu, c, fails, nan=True)
    _finish(fails)


# ---------------------------------------------------------------- (b) uniform
@pytest.mark.parametrize("name", NAMES)
def test_uniform(gpu, name):
    fails = []
    for c in _cells(name):
        L = Launch(gpu, c)
        g = L.hq // L.hkv
        for i, pos in enumerate(_sets(L, c, "uniform")):
            tag = f"{R.cell_id(c)} uniform pos {pos}"
            q, Kc, Vc, V = R.uniform(pos, L.hq, L.hkv, L.hd, L.T, L.kv, _seed(c, "uniform", i))
            L.load(q, Kc, Vc, pos)
            r = L.twice(fails, tag)
            parts, ns, ppwg = L.parts(r), L.ns(), L.plan["ppwg"]
            for h in range(L.H):
                b = h // L.hq
                kvh, p = b * L.hkv + (h % L.hq) // g, pos[b]
                assert np.abs(V[kvh, :p + 1]).sum(axis=0).max() < 2 ** 24
                ref = V[kvh, :p + 1].sum(axis=0) / (p + 1)
                if L.plan["merge"] != 1:
                    got = r["out"][h * L.hd:(h + 1) * L.hd]
                    if (p + 1) & p == 0:
                        if not np.array_equal(got, ref.astype(np.float32)):
                            fails.append(f"{tag}: head {h}: out is not sum V / 2^k exactly")
                    elif not (np.abs(got.astype(np.float64) - ref) <= np.spacing(np.abs(ref).astype(np.float32))).all():
                        fails.append(f"{tag}: head {h}: out more than an ulp from sum V / (pos + 1)")
                for s in range(ns[h]):
                    lo, hi = s * ppwg, min((s + 1) * ppwg, p + 1)
                    row = parts[h, s]
                    if row[L.hd + 1] != hi - lo or row[L.hd] != 0 or \
                            not np.array_equal(row[:L.hd], V[kvh, lo:hi].sum(axis=0)):
                        fails.append(f"{tag}: head {h} split {s}: (m, l) = ({row[L.hd]}, {row[L.hd + 1]}) for (0, "
                                     f"{hi - lo}), or o is not the integer sum")
    _finish(fails)


# ---------------------------------------------------------------- (c) realistic
@pytest.mark.parametrize("name", NAMES)
def test_realistic(gpu, name):
    fails = []
    for c in _cells(name):
        L = Launch(gpu, c)
        for i, pos in enumerate(_sets(L, c, "real")):
            tag = f"{R.cell_id(c)} real pos {pos}"
            q, Kc, Vc, scaled = R.realistic(pos, L.hq, L.hkv, L.hd, L.T, L.kv, L.plan, _seed(c, "real", i))
            L.load(q, Kc, Vc, pos)
            r = L.twice(fails, tag)
            K, V = _live(R.values(Kc, L.kv), pos, L.hkv), _live(R.values(Vc, L.kv), pos, L.hkv)
            ns = L.ns()
            ref = R.decode(q, K, V, pos, L.hq, L.hkv, L.hd)
            tol, _ = R.real_tol(q, K, V, pos, L.hq, L.hkv, L.hd, ns)
            sc = np.repeat(scaled, L.hd)
            bar = np.where(sc, tol, R.ATOL + R.RTOL * np.abs(ref))
            got = _merged(L, r) if L.plan["merge"] == 1 else r["out"][:L.n].astype(np.float64)
            with np.errstate(invalid="ignore"):
                _hold(fails, tag + " out", got, ref, bar)
                err = np.abs(got - ref)
            _ratio((name, "scaled"), err[sc], tol[sc])
            _ratio((name, "unscaled, of 1e-5"), err[~sc], bar[~sc])
            parts = L.parts(r).astype(np.float64)
            for s in range(L.plan["max_splits"]):
                m, lse, on = R.split_state(q, K, V, pos, L.hq, L.hkv, L.hd, L.plan["ppwg"], s)
                live = ns > s
                if not live.any():
                    continue
                ts, tl = R.real_tol(q, K, V, pos, L.hq, L.hkv, L.hd, ns, split=(L.plan["ppwg"], s))
                ts = ts.reshape(L.H, L.hd)
                row = parts[live, s]
                o_l = row[:, :L.hd] / row[:, L.hd + 1:L.hd + 2]
                with np.errstate(invalid="ignore", divide="ignore"):
                    glse = row[:, L.hd] + np.log(row[:, L.hd + 1])
                bar_s = np.where(scaled[live][:, None], ts[live], R.ATOL + R.RTOL * np.abs(on[live]))
                _hold(fails, f"{tag} split {s} o / l", o_l, on[live], bar_s)
                _hold(fails, f"{tag} split {s} m + log l", glse, lse[live], tl[live])
                _ratio((name, "partial m + log l"), np.abs(glse - lse[live]), tl[live])
    _finish(fails)


# ---------------------------------------------------------------- (e) the same bits by another way
def _real_launch(L, c, i=0):
    pos = (_sets(L, c, "needle") + _sets(L, c, "uniform"))[i]
    q, Kc, Vc, _ = R.realistic(pos, L.hq, L.hkv, L.hd, L.T, L.kv, L.plan, _seed(c, "real", i))
    L.load(q, Kc, Vc, pos)
    return pos, q


def test_device_cus_is_cus_0(gpu):
    """cus = the device's compute unit count is cus = 0: the same plan and the same bits."""
    fails = []
    ncu = gpu.cuda.get_device_properties(0).multi_processor_count
    for name in NAMES:
        for c in _cells(name)[:2]:
            a, b = Launch(gpu, c, cus=0), Launch(gpu, c, cus=ncu)
            if {k: v for k, v in a.plan.items() if k != "cus"} != {k: v for k, v in b.plan.items() if k != "cus"}:
                fails.append(f"{R.cell_id(c)}: plan at cus 0 {a.plan}, at the device's {b.plan}")
                continue
            _real_launch(a, c)
            _real_launch(b, c)
            ra, rb = a.twice(fails, R.cell_id(c) + " cus 0"), b.twice(fails, R.cell_id(c) + f" cus {ncu}")
            if not (_bits_equal(ra["out"], rb["out"]) and _bits_equal(ra["part"], rb["part"])):
                fails.append(f"{R.cell_id(c)}: cus {ncu} and cus 0 differ")
    _finish(fails)


def test_in_launch_merge_is_the_merge_launch(gpu):
    """R4: the last-arriving workgroup's merge (0) and attn_merge_kernel (2) both merge in split order: the same bits."""
    fails = []
    cells = _cells("R4")
    for c0 in [c for c in cells if c["merge"] == 0]:
        c2 = [c for c in cells if c["merge"] == 2 and (c["hq"], c["T"]) == (c0["hq"], c0["T"])][0]
        for i in range(3):
            a, b = Launch(gpu, c0), Launch(gpu, c2)
            _real_launch(a, c0, i)  # (seeded by c0 for both: the same inputs)
            pos, _ = _real_launch(b, c0, i)
            assert (a.plan["merge"], b.plan["merge"], b.plan["merge_grid"] > 0) == (0, 2, True)
            assert (a.plan["g"], a.plan["kv_group"], a.plan["grid"]) == (b.plan["g"], b.plan["kv_group"], b.plan["grid"])
            ra, rb = a.twice(fails, R.cell_id(c0)), b.twice(fails, R.cell_id(c2))
            if not (_bits_equal(ra["out"], rb["out"]) and _bits_equal(ra["part"], rb["part"])):
                fails.append(f"{R.cell_id(c0)} pos {pos}: merge 0 and merge 2 differ")
    _finish(fails)


def test_entry_is_mha_strided(gpu):
    """M3: batch 1, merge 0, fp16, cus 0: the new entry and ops.mha_strided on the same buffers, bit for bit."""
    from simplellminference_amd import ops
    fails = []
    for c in _cells("M3"):
        L = Launch(gpu, c)
        assert (L.plan["kernel"], L.plan["merge"], c["cus"]) == (1, 0, 0)
        for i in range(2 * R.n_sets(1)):  # (every listed position)
            pos, _ = _real_launch(L, c, i)
            r = L.twice(fails, R.cell_id(c))
            ref = ops.mha_strided(L.qd, L.kd[1], L.vd[1], pos[0], L.T, L.hd, L.hq, L.hkv, L.hd, L.T * L.hd)
            if not _bits_equal(ref.cpu().numpy(), r["out"][:L.n]):
                fails.append(f"{R.cell_id(c)} pos {pos}: sli_decode_attn and sli_mha_strided differ")
    _finish(fails)


def test_cus_above_the_device_is_refused(gpu):
    """cus = the device's compute units + 1 is refused on the host (nothing is launched), by the plan and the launch."""
    from simplellminference_amd import _lib, ops
    ncu = gpu.cuda.get_device_properties(0).multi_processor_count
    c = _cells("M3")[0]
    assert ncu + 1 <= 4096
    L = Launch(gpu, c, cus=ncu)
    _real_launch(L, c)
    L.cus = ncu + 1
    with pytest.raises(_lib.SliError, match="cus exceeds the device's compute units") as e:
        L.run()
    assert e.value.code == 1
    # (the plan needs no device for cus != 0, so it cannot know the device's count: it takes ncu + 1)
    assert ops.decode_attn_plan(R.DT[c["kv"]], c["B"], c["hq"], c["hkv"], c["hd"], c["T"], cus=ncu + 1)["cus"] == ncu + 1


def test_zz_report(gpu):
    """Prints the largest error / bound per cell class (run with -s): the figures of the docstring."""
    for k in sorted(RATIOS):
        print(f"decode_attn ratio {k}: {RATIOS[k]:.4f}")
