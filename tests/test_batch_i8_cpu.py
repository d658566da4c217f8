"""The int8 batched projection's host-side interface (sli_matmul_batch_i8): symbols, the workspace sizes and the
argument checks that need no device."""
import ctypes

import pytest


@pytest.fixture(scope="module")
def lib():
    from simplellminference_amd import _lib
    return _lib.load()


def test_symbols_exist(lib):
    assert hasattr(lib, "sli_matmul_batch_i8_workspace_bytes")
    assert hasattr(lib, "sli_matmul_batch_i8")
    from simplellminference_amd import _lib
    assert {"sli_matmul_batch_i8_workspace_bytes", "sli_matmul_batch_i8"} <= set(_lib.exported_symbols())


@pytest.mark.parametrize("tiled", [0, 1])
def test_workspace_zero_for_unsupported_shapes(lib, tiled):
    ws = lib.sli_matmul_batch_i8_workspace_bytes
    assert ws(64, 128, 8, tiled) > 0
    assert ws(64, 100, 8, tiled) == 0  # cols % 32 != 0
    assert ws(64, 128, 9, tiled) == 0  # batch > 8
    assert ws(64, 128, 0, tiled) == 0  # batch < 1
    assert ws(64, 128, -1, tiled) == 0


@pytest.mark.parametrize("rows,cols,batch", [(64, 128, 8), (100, 96, 3)])
def test_tiled_workspace_holds_the_image(lib, rows, cols, batch):
    """tiled = 1 adds the fragment-layout image: ceil(rows / 16) tiles x cols / 32 blocks x 512 bytes."""
    ws = lib.sli_matmul_batch_i8_workspace_bytes
    image = ((rows + 15) // 16) * (cols // 32) * 512
    assert image >= rows * cols
    assert ws(rows, cols, batch, 1) >= ws(rows, cols, batch, 0) + image
    assert ws(rows, cols, batch, 0) == lib.sli_matmul_batch_workspace_bytes(rows, cols, batch)


def test_fp16_entry_still_rejects_int8(lib):
    """sli_matmul_batch checks its arguments before it touches the device: SLI_DT_I8 is SLI_ERR_ARG."""
    from simplellminference_amd._lib import DT_I8
    buf = (ctypes.c_char * 4096)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    rc = lib.sli_matmul_batch(p, p, DT_I8, p, 16, 32, 1, p, 4096, None)
    assert rc == 1  # SLI_ERR_ARG
