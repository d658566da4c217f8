"""The prefill GEMM's LDS-DMA piece addresses on the host: tests/cpp/pgemm_pieces.cpp enumerates every piece of every
stage and lane for every tiling prefill.h pg_pick returns and K in {64, 128, 192, 320, 704}, through the very
__host__ __device__ functions the kernel's setup loop calls (pg_piece, PgGeo::piece / dst). It checks that every source
range stays inside its own row and that every byte of every valid k-block lands where the fragment reads expect it."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "simplellminference_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "cpp", "pgemm_pieces.cpp")
BIN = os.path.join(ROOT, "tests", "cpp", "_build", "pgemm_pieces")


def _compile():
    deps = [SRC] + [os.path.join(CSRC, h) for h in os.listdir(CSRC) if h.endswith(".h")]
    if os.path.exists(BIN) and os.path.getmtime(BIN) >= max(os.path.getmtime(d) for d in deps):
        return BIN
    os.makedirs(os.path.dirname(BIN), exist_ok=True)
    cmd = ["hipcc", "--offload-arch=gfx950", "-O1", "-std=c++17", f"-I{CSRC}", SRC, "-o", BIN]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return BIN


def test_every_piece_stays_in_its_row_and_lands_where_the_fragment_reads_expect():
    r = subprocess.run([_compile()], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "pieces ok" in r.stdout
