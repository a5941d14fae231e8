"""The LDS-staged table kernel's chunk -> (box row, column) split (csrc/gs360_tablestage.hip), restated in NumPy with the kernel's 32-bit
arithmetic and checked against divmod for every chunk of every box the LDS budget admits.  No GPU: this guards the arithmetic wherever the
suite runs; tests/test_tablestage_limits_gpu.py runs the same boxes through the kernel."""
import re

import numpy as np

from conftest import PKG

CSRC = PKG / "csrc"


def _budget():
    m = re.search(r"constexpr int kTsBoxBudget = ([0-9 *+-]+);", (CSRC / "gs360_capi_remap.hip").read_text())
    return eval(m.group(1), {"__builtins__": {}})     # (a constant expression of literals)


def _max_dim():
    return int(re.search(r"constexpr int kMapPlanMaxDim = (\d+);", (CSRC / "gs360_kernels.h").read_text()).group(1))


def split(cc, wch, bits):
    """table_stage_plan_kernel's magic (gs360_tablestage.hip:121) and box_load's chunk() (:233) on int64 chunk indices cc, with `bits` = 21"""
    magic = ((1 << bits) + wch - 1) // wch
    row = ((cc.astype(np.uint32) * np.uint32(magic)) >> np.uint32(bits)).astype(np.int64)      # (uint32_t)cc * (uint32_t)T.magic >> 21
    return row, cc - row * wch, magic


def test_kernel_has_the_restated_split():
    src = (CSRC / "gs360_tablestage.hip").read_text()
    assert "T.magic = ((1 << 21) + T.wch - 1) / T.wch;" in src
    assert "const int row = (int)(((uint32_t)cc * (uint32_t)T.magic) >> 21), col = cc - row * T.wch;" in src


def test_row_split_exact_for_every_admitted_box():
    budget_chunks, W = _budget() // 16, _max_dim()
    max_wch = ((((3 * (W - 1)) & ~3) + 12) + 15) >> 4    # a box from column 0 to W - 1 (gs360_tablestage.hip:108-109)
    assert (budget_chunks, max_wch) == (1660, 766)
    wrong20 = set()
    for wch in range(1, max_wch + 1):
        for nrows in range(2, budget_chunks // wch + 1):
            cc = np.arange(nrows * wch, dtype=np.int64)
            row, col, magic = split(cc, wch, 21)
            assert int(cc[-1]) * magic < 1 << 32, (wch, nrows)                                  # no 32-bit wrap
            assert np.array_equal(row, cc // wch) and np.array_equal(col, cc % wch), (wch, nrows)
            if not np.array_equal(split(cc, wch, 20)[0], cc // wch):
                wrong20.add((wch, nrows))
    # the 20-bit magic the kernel had before put chunk 2 wch - 1 of these boxes into row 2, column -1
    assert wrong20 == {(756, 2), (762, 2)}
