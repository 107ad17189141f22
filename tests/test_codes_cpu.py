"""The step-mode, matrix-core-mode, flag and inner-order codes of
csrc/include/svdj_hip.h, read from the header's text (no GPU, no library
load), pinned to their historical values and to ops/kernels.py's constants."""
import re
from pathlib import Path

import svdj

K = svdj.ops.kernels
HEADER = Path(svdj.__file__).resolve().parent / "csrc" / "include" / "svdj_hip.h"
# the numeric values of the C ABI: no pull request changes them
HISTORICAL = {
    "SVDJ_STEP_CROSS": 0, "SVDJ_STEP_FULL": 1, "SVDJ_STEP_CROSS_BIP": 2,
    "SVDJ_STEP_CROSS_ONLY": 3, "SVDJ_STEP_QUAD": 4, "SVDJ_STEP_QUAD_SECOND": 5,
    "SVDJ_MMA_NATIVE": 0, "SVDJ_MMA_BF16X6": 1, "SVDJ_MMA_BF16X3": 2,
    "SVDJ_MMA_MASK": 0xff, "SVDJ_STEPS_GRAM2": 256, "SVDJ_STEPS_SHARED_GPU": 512,
    "SVDJ_INNER_CYCLIC": 0, "SVDJ_INNER_BIPARTITE": 1, "SVDJ_INNER_CROSS": 2,
    "SVDJ_INNER_AUTO": 3,
}


def header_codes():
    """{name: value} of every `SVDJ_X = <integer>` enumerator in the header,
    comments stripped."""
    text = re.sub(r"//[^\n]*", "", HEADER.read_text())
    found = re.findall(r"\b(SVDJ_[A-Z0-9_]+)\s*=\s*(0[xX][0-9a-fA-F]+|\d+)\s*[,}]", text)
    codes = {name: int(value, 0) for name, value in found}
    assert len(codes) == len(found), "a code is defined twice"
    return codes


def test_header_codes_keep_their_historical_values():
    assert header_codes() == HISTORICAL


def test_python_constants_equal_the_header():
    h = header_codes()
    for name in ("STEP_CROSS", "STEP_FULL", "STEP_CROSS_BIP", "STEP_CROSS_ONLY", "STEP_QUAD",
                 "STEP_QUAD_SECOND", "MMA_MASK", "STEPS_GRAM2", "STEPS_SHARED_GPU"):
        assert getattr(K, name) == h["SVDJ_" + name], name
    assert K.MMA_CODES == {"native": h["SVDJ_MMA_NATIVE"], "bf16x6": h["SVDJ_MMA_BF16X6"],
                           "bf16x3": h["SVDJ_MMA_BF16X3"]}
    assert all(code & ~h["SVDJ_MMA_MASK"] == 0 for code in K.MMA_CODES.values())
    # block_solve passes INNER_ORDERS.index(name); "auto" follows the named orders
    assert [K.INNER_ORDERS.index(n) for n in ("cyclic", "bipartite", "cross")] == [
        h["SVDJ_INNER_CYCLIC"], h["SVDJ_INNER_BIPARTITE"], h["SVDJ_INNER_CROSS"]]
    assert h["SVDJ_INNER_AUTO"] == len(K.INNER_ORDERS)


def test_step_modes_maps_inner_orders_to_the_cross_modes():
    plan = [K.STEP_FULL, K.STEP_CROSS, K.STEP_QUAD, K.STEP_QUAD_SECOND]
    for order, cross in (("cyclic", K.STEP_CROSS), ("bipartite", K.STEP_CROSS_BIP),
                         ("cross", K.STEP_CROSS_ONLY)):
        assert K.step_modes(plan, order) == [K.STEP_FULL, cross, K.STEP_QUAD, K.STEP_QUAD_SECOND]
