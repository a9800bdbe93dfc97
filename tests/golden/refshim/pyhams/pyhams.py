"""Stand-in for pyHAMS (absent from the image), used ONLY by tests/golden/make_bem_golden.py
to run the read-only reference on WAMIT-format coefficient files.  read_wamit1 / read_wamit3
are the project's own reader (raft-teststuff_amd/raft/bem_io.py, loaded by file path: the name
`raft` is the reference package there), so the reference's readHydro / calcBEM / excitation
code runs on the same parsed arrays as the product.  Running HAMS is not provided."""
import importlib.util
import os

_ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))))
_spec = importlib.util.spec_from_file_location("rh_bem_io", os.path.join(_ROOT, "raft-teststuff_amd", "raft", "bem_io.py"))
_mod = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_mod)

read_wamit1 = _mod.read_wamit1
read_wamit3 = _mod.read_wamit3


def run_hams(*a, **kw):
    raise NotImplementedError("the pyHAMS stand-in only reads WAMIT-format files")
