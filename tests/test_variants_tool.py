"""tools/ubench/variants.py builds its timing-only libraries by replacing text in copies of the kernel
sources.  An anchor that has drifted away from the sources makes an entry unbuildable (or, found twice,
ambiguous), and nothing else notices.  Reads text only, compiles nothing."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools", "ubench"))
import variants  # noqa: E402

# the timing ablations that were `#if RH_ABL_*` blocks of the kernels live on as entries
RETIRED_ABLATIONS = ("cNoLoad", "cNoComp", "aNoLoad", "aNoComp", "aNoBfly", "gNoPot", "gNoBil", "gNoPch", "gNoStore",
                     "gNoMirror", "gNoKay", "gNoCoef")


def test_every_anchor_occurs_exactly_once():
    bad = []
    for name, edits in variants.EDITS.items():
        for fname, anchor, replacement in edits:
            with open(os.path.join(variants.CSRC, fname)) as fh:
                n = fh.read().count(anchor)
            if n != 1 or replacement == anchor:
                bad.append((name, fname, n, anchor[:60]))
    assert not bad, bad
    assert all(variants.EDITS.get(n) for n in RETIRED_ABLATIONS)
