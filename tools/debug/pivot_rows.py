"""Which rows does the 6 x 6 LU of the solve kernels pivot to on real impedance matrices?  (CPU only.)

rh::lu_solve<6> (csrc/rh_device.h) exchanges rows with per-lane selects, and a wave runs the selects of
step k with candidate row i only if one of its lanes pivots there.  What that costs depends on the data.
This tool runs the CPU oracle (oracle/raft_oracle.solve_dynamics) on a golden table for a seeded list of
sea states (bench.sea_states), eliminates every converged Z (one per case and bin) with the kernel's
rule -- partial pivoting by max |re| + |im|, the first maximum wins -- and prints

  * the pivot row of every step, counted over all (case, bin) systems;
  * the select instructions of one wave's LU, averaged over the waves, with lane = bin as the kernels
    map them (a wave is 64 consecutive bins; the pad lanes of the last wave repeat its last bin):
      chain     one test per step, then the selects of every candidate row k+1 .. 5
                (lu_solve<6, false>);
      per row   one test per candidate row (lu_solve<6, true>).
    Exchanging rows k and i takes 8 (7 - k) selects: 6 - k columns and the right-hand side, two
    doubles each, in both directions, two 32-bit selects a double.

Usage: python tools/debug/pivot_rows.py c2 | c4 [--ncase 6] [--seed S]
  c2  tests/golden/c2_nw1000.npz (nw = 1000), seed 20241016 as the bench's C2 leg
  c4  tests/golden/c4_farm.npz, FOWT 0 (nw = 240), seed 20241020 as the bench's C4 leg
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
WAVE = 64


def tables(which):
    if which == "c2":
        T = dict(np.load(os.path.join(ROOT, "tests", "golden", "c2_nw1000.npz")))
        return T, int(T["nIter"]), float(T["XiStart"]), 20241016
    G = dict(np.load(os.path.join(ROOT, "tests", "golden", "c4_farm.npz")))
    T = {k[3:]: v for k, v in G.items() if k.startswith("f0_")}
    return T, int(G["nIter"]), float(G["XiStart"]), 20241020


def pivot_rows(Z):
    """[nw][5]: the row every step 0..4 pivots to, for Z [nw][6][6] (the kernel's rule)."""
    A = np.array(Z, dtype=complex)
    nw = len(A)
    out = np.zeros([nw, 5], dtype=int)
    ar = np.arange(nw)
    for k in range(5):
        v = np.abs(A[:, k:, k].real) + np.abs(A[:, k:, k].imag)
        p = k + np.argmax(v, axis=1)                    # argmax: the first maximum
        out[:, k] = p
        rk, rp = A[ar, k].copy(), A[ar, p].copy()
        A[ar, k], A[ar, p] = rp, rk
        l = A[:, k + 1:, k] / A[:, k, k][:, None]
        A[:, k + 1:, k:] -= l[:, :, None] * A[:, k, None, k:]
    return out


def selects(piv):
    """(chain, per row) select instructions of each wave's LU, for piv [nw][5] of one case."""
    chain, rows = [], []
    for w0 in range(0, len(piv), WAVE):
        pw = piv[w0:w0 + WAVE]
        c = r = 0
        for k in range(5):
            per = 8 * (7 - k)
            off = set(pw[:, k]) - {k}
            c += per * (5 - k) if off else 0
            r += per * len(off)
        chain.append(c)
        rows.append(r)
    return chain, rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("which", choices=["c2", "c4"])
    ap.add_argument("--ncase", type=int, default=6)
    ap.add_argument("--seed", type=int, default=None)
    args = ap.parse_args()
    import bench
    from oracle import raft_oracle as O
    T, nIter, XiStart, seed = tables(args.which)
    seed = seed if args.seed is None else args.seed
    cases = bench.sea_states(args.ncase, seed)
    nw = len(T["w"])
    count = np.zeros([5, 6], dtype=int)
    chain, rows = [], []
    iters = []
    for c in cases:
        r = O.solve_dynamics(T, dict(c), nIter, XiStart)
        iters.append(int(r["iters"]))
        piv = pivot_rows(np.moveaxis(r["Z"], 2, 0))
        for k in range(5):
            count[k] += np.bincount(piv[:, k], minlength=6)
        c_, r_ = selects(piv)
        chain += c_
        rows += r_
    print(f"# tools/debug/pivot_rows.py {args.which}: nw = {nw}, {args.ncase} sea states of bench.sea_states({args.ncase}, {seed}), "
          f"oracle iterations {iters}")
    print(f"# pivot row per step over the {args.ncase * nw} (case, bin) systems (row: bins)")
    for k in range(5):
        order = sorted(range(6), key=lambda i: -count[k][i])
        print(f"step {k}: " + ", ".join(f"row {i}: {count[k][i]}" for i in order if count[k][i]))
    print(f"# select instructions per wave-LU, mean over {len(chain)} waves of {WAVE} bins (lane = bin)")
    print(f"chain (one test per step):   {np.mean(chain):7.1f}   min {min(chain)} max {max(chain)}")
    print(f"per row (one test per row):  {np.mean(rows):7.1f}   min {min(rows)} max {max(rows)}")
    print(f"saved per wave-LU:           {np.mean(chain) - np.mean(rows):7.1f}")


if __name__ == "__main__":
    main()
