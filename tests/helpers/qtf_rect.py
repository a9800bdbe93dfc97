"""Shared by tests/test_oracle_qtf.py and tests/test_gpu_qtf_rect.py: the layout of
tests/golden/qtf_rect.npz (make_golden.py golden_qtf_rect)."""
import numpy as np

DESIGNS = {"A": "VolturnUS-S_example", "B": "VolturnUS-S_rectcols"}
# (key of the reference QTF, index into qtf_betas, moving body?)
RUNS = [("b0", 0, True), ("b30", 1, True), ("b30_fixed", 2, False)]
RUN_IDS = [r[0] for r in RUNS]


def rect_tables(R, tag):
    """Design tables (the keys make_golden.design_tables writes) of design A or B."""
    pre = tag + "_"
    return {k[len(pre):]: v for k, v in R.items() if k.startswith(pre) and "_qtf_" not in k}


def rao_of(R, moving):
    return R["qtf_X"] if moving else np.zeros_like(R["qtf_X"])
