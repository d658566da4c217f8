"""The decode kernels' leading plain arguments (the hot block, gemv.h gemv_kernel) must arrive preloaded in SGPRs:
the build's -amdgpu-kernarg-preload-count only preloads a kernel's leading run of pointer / integer arguments and
stops at the first by-value struct, so a struct moved in front of the run (or the flag lost from the build) would
silently put the kernarg load back on the path to every wave's first memory request.

CPU only: hipcc cross-compiles engine.hip and ops.hip device-only to assembly with the build's own flags, and the
test reads one directive of each kernel descriptor, `.amdhsa_user_sgpr_kernarg_preload_length`, nothing else.
"""
import concurrent.futures as cf
import os
import re
import subprocess

import pytest

from simplellminference_amd import build as B

# kernel name in the mangled symbol -> dwords of its leading plain arguments
#   gemv_kernel        W, x, norm_w (6), cols, csplit, cw, nunits, cpp, tw_m, cw_m, div_sh (8)
#   gemv_sum_kernel    W, x, norm_w, parts (8), cols, cw, nunits, tw_m, cw_m, div_sh (6)
#   gemv_merge_kernel  W, part, pos_dev (6), cols, cw, nunits, tw_m, cw_m, div_sh, max_splits, hd (8)
#   embedding_kernel   token_host + pad (2), token_dev, table, row_scale, out (8), vocab, dim (2): every argument
#   keyreduce_kernel   keys (2), n + pad (2), st, prompt, hist (6), T (1): every argument
# (attn_partial_kernel keeps its single by-value struct: preloading its arguments measured no gain)
HOT_DWORDS = {"11gemv_kernelI": 14, "15gemv_sum_kernelI": 14, "17gemv_merge_kernelI": 14, "16embedding_kernelI": 12,
              "16keyreduce_kernelI": 11}


def _device_asm(src, out):
    cmd = ["hipcc", *B.CXXFLAGS, "--cuda-device-only", "-S", os.path.join(B.CSRC, src), "-o", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        pytest.fail(f"device-only compile of {src} failed:\n{r.stderr[-2000:]}")
    return out.read_text()


def test_hot_block_is_preloaded(tmp_path):
    with cf.ThreadPoolExecutor(2) as ex:
        texts = list(ex.map(lambda s: _device_asm(s, tmp_path / (s + ".s")), ["engine.hip", "ops.hip"]))
    found = {k: 0 for k in HOT_DWORDS}
    for text in texts:
        for m in re.finditer(r"\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel", text, re.S):
            name, desc = m.group(1), m.group(2)
            for needle, want in HOT_DWORDS.items():
                if needle not in name:
                    continue
                got = re.search(r"\.amdhsa_user_sgpr_kernarg_preload_length\s+(\d+)", desc)
                assert got, f"{name}: no kernarg preload directive"
                assert int(got.group(1)) >= want, f"{name}: {got.group(1)} dwords preloaded, hot block is {want}"
                found[needle] += 1
    assert all(found.values()), f"kernels not found in the device code: {[k for k, v in found.items() if not v]}"
