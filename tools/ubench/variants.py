"""Build phase-ablated copies of librafthip.so (tools/ubench/var_<name>.so) to attribute the
case-solve time to its phases on the GPU.  The ablated libraries give wrong answers by
construction; tools/ubench/time_solve.py only times them (per executed iteration)."""
import os
import shutil
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import __graft_entry__ as G  # noqa: E402  (the build's translation units and their flags)
REL_CSRC = os.path.relpath(G.CSRC, ROOT)
CSRC = G.CSRC

# name: [(file under csrc, anchor, replacement)]; every anchor occurs exactly once in its file
# (tests/test_variants_tool.py).  The entries from cNoLoad on are the timing ablations that were `#if
# RH_ABL_<PHASE>_<WHAT>` blocks of the kernels (DESIGN.md §5 records their numbers).  The first letter
# says which driver times a library: q, k, g the QTF ones (run_qtf_variants.sh, run_qtf_mfma_variants.sh).
EDITS = {
    "qNoPot": [("rh_qtf.hip", "    if (pot_on && rz <= 0) {", "    if (pot_on && rz <= -1e300) {")],
    "qNoKY": [("rh_qtf.hip", "    for (int ir = NWV - 1 - wv; ir < q.nkr; ir += NWV) {", "    for (int ir = NWV - 1 - wv; ir < 0; ir += NWV) {")],
    "qNoRot": [("rh_qtf.hip", "    // (5) Rainey body-rotation terms (:1556-1575)\n    cd fr[3];\n    {", "    // (5) Rainey body-rotation terms (:1556-1575)\n    cd fr[3] = {vA[0], vA[1], vA[2]};\n    if (rz < -1e300) {")],
    # MFMA QTF path (rh_qtf_mfma.hip)
    "kNoMfma": [("rh_qtf_mfma.hip", "          ca = mfma64(va[s], vr[s], ca);\n          cbk = mfma64(vb[s], vr[s], cbk);",
                 "          ca[0] += va[s] * vr[s];\n          cbk[0] += vb[s] * vr[s];")],
    "prof": [],          # unmodified source built with -DRH_PROF (phase cycle counters)
    # k_solve_lds, phase C: the ring keeps its first nodes / the loads consumed with one add each
    "cNoLoad": [("rh_solve.hip", "        const unsigned so = (unsigned)(n < nn ? n : nn - 1) * 3u * nw16;\n#pragma unroll\n        for (int p = 0; p < 2; ++p) K[p] = bld(bK, vj, so + (unsigned)(p + 1) * nw16);",
                      "        const unsigned so = (unsigned)(n < nn ? n : nn - 1) * 3u * nw16;\n        if (n >= kRingC) return;\n#pragma unroll\n        for (int p = 0; p < 2; ++p) K[p] = bld(bK, vj, so + (unsigned)(p + 1) * nw16);")],
    "cNoComp": [("rh_solve.hip", "        S1 = add(S1, scl(K[0], a1));\n        S2 = add(S2, scl(K[1], a2));\n        T1 = add(T1, scl(K[0], a3));",
                      "        S1 = add(S1, K[0]); S2 = add(S2, K[1]);\n        load1(K, n + kRingC);\n        return;\n"
                      "        S1 = add(S1, scl(K[0], a1));\n        S2 = add(S2, scl(K[1], a2));\n        T1 = add(T1, scl(K[0], a3));")],
    # ... phase A: the same two, and the node sums without their butterfly (the two-pass kernel's tbfly3 only)
    "aNoLoad": [("rh_solve.hip", "      auto load_node = [&](cd (&K)[2][NB], int n) {\n        const unsigned so = (unsigned)(n < nn ? n : nn - 1) * 3u * nw16;\n",
                      "      auto load_node = [&](cd (&K)[2][NB], int n) {\n        const unsigned so = (unsigned)(n < nn ? n : nn - 1) * 3u * nw16;\n        if (n >= kRingA) return;\n")],
    "aNoComp": [("rh_solve.hip", "        s1 = s2 = 0;\n#pragma unroll\n        for (int j = 0; j < NB; ++j) {\n          const double z = bz[j];",
                      "        s1 = s2 = 0;\n#pragma unroll\n        for (int j = 0; j < NB; ++j) { s1 += K[0][j].r + K[0][j].i; s2 += K[1][j].r + K[1][j].i; }\n        return;\n"
                      "#pragma unroll\n        for (int j = 0; j < NB; ++j) {\n          const double z = bz[j];")],
    "aNoBfly": [("rh_solve.hip", "            const double tot = tbfly3(s1, s2, 0.0);", "            const double tot = s1 + s2;")],
    # k_qtf_gemm: no pair scalars of the potential, no bilinear / no potential-channel k-steps, no stores,
    # the upper triangle only
    "gNoPot": [("rh_qtf_mfma.hip", "      qtf_pot_scalars(q.w2[i1], q.k2[i1], tkh[x >> 4], q.w2[i2], q.k2[i2], tkh[16 + (x & 15)], cb, sb, h, g, sp, sm);",
                     "      sp = cd{q.w2[i1], tkh[x >> 4]}; sm = cd{q.w2[i2], tkh[16 + (x & 15)]};")],
    "gNoBil": [("rh_qtf_mfma.hip", "wk.R + ((size_t)4 * k0 + kr) * n2p + i2b + mr, nk,\n", "wk.R + ((size_t)4 * k0 + kr) * n2p + i2b + mr, 0,\n")],
    "gNoPch": [("rh_qtf_mfma.hip", "kq / 4, step, p1, p2, p3, c1, c2, c3);", "0, step, p1, p2, p3, c1, c2, c3);")],
    "gNoStore": [("rh_qtf_mfma.hip", "    rh_c128* up = qtf + ((size_t)i1 * n2 + i2) * 6 + d;\n    if (!mirror) {",
                       "    rh_c128* up = qtf + ((size_t)i1 * n2 + i2) * 6 + d;\n    if (Qf.r == 1.2345e300) st(up, Qf);\n    continue;\n    if (!mirror) {")],
    "gNoMirror": [("rh_qtf_mfma.hip", "    rh_c128* up = qtf + ((size_t)i1 * n2 + i2) * 6 + d;\n    if (!mirror) {",
                        "    rh_c128* up = qtf + ((size_t)i1 * n2 + i2) * 6 + d;\n    st(up, Qf);\n    continue;\n    if (!mirror) {")],
    # k_qtf_lk's launch: no Kim & Yue tiles / no coefficient blocks
    "gNoKay": [("rh_abi.hip", "      if (cached) nkb = 0;   // their tile sums KS are in the workspace already\n", "      nkb = 0;\n")],
    "gNoCoef": [("rh_abi.hip", "      int nkb = (blocks + per - 1) / per, nly = 18 + q->nq + q->nmq;\n", "      int nkb = (blocks + per - 1) / per, nly = 0;\n")],
}


def build(name, edits, flags=()):
    """Copy the sources, apply the edits and build tools/ubench/var_<name>.so as the library itself is built."""
    tmp = tempfile.mkdtemp()
    for rel in (REL_CSRC, "include"):   # (csrc includes the header by relative path)
        shutil.copytree(os.path.join(ROOT, rel), os.path.join(tmp, rel))
    for fname, a, b in edits:
        p = os.path.join(tmp, REL_CSRC, fname)
        with open(p) as fh:
            s = fh.read()
        assert s.count(a) == 1, (name, fname, a[:60])
        with open(p, "w") as fh:
            fh.write(s.replace(a, b))
    out = os.path.join(ROOT, "tools", "ubench", f"var_{name}.so")
    csrc, G.CSRC = G.CSRC, os.path.join(tmp, REL_CSRC)   # compile_library: the shipped units and flags
    try:
        G.compile_library(out, list(flags))
    finally:
        G.CSRC = csrc
        shutil.rmtree(tmp)
    print("built", out)


if __name__ == "__main__":
    names = sys.argv[1:] or list(EDITS)
    for n in names:
        base = n[:-5] if n.endswith("+prof") else n
        build(n.replace("+", "_"), EDITS[base], ["-DRH_PROF"] if (n == "prof" or n.endswith("+prof")) else [])
