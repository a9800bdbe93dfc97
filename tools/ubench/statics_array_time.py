"""Time the mean-offset statics of N cases on VolturnUS-S_farm (two FOWTs, shared line with two
clump-weight free points; current speed U(0, 1) m/s, heading U(0, 360) deg, seeded):
  (a) the host path: a Python loop of Model.solveStatics plus the array system's analytic
      stiffness and central-difference tension Jacobian (24 perturbed free-point equilibria) at
      each offset pose, every case on a fresh copy of the state at the reference poses;
  (b) Model.solveStaticsArrayBatch: the wall time of the whole call (host F_env of every case and
      FOWT, uploads, two launches, downloads) and the HIP-event time of the two launches alone
      (rh_array_statics_solve, rh_moor_array_eval with the Jacobian).
Warm-up calls first; medians over the repeats, with the spread.  usage: statics_array_time.py [N] [out.txt]"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "raft-teststuff_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main(n, out_path=None):
    import torch
    import raft
    from conftest import load_design
    from raft.mooring_array_device import DeviceArrayMooring
    rng = np.random.default_rng(64)
    base = {"wind_speed": 0, "wind_heading": 0, "turbulence": 0, "turbine_status": "operating", "yaw_misalign": 0,
            "wave_spectrum": "JONSWAP", "wave_period": 0, "wave_height": 0, "wave_heading": 0}
    cases = [dict(base, current_speed=float(u), current_heading=float(h))
             for u, h in zip(rng.uniform(0, 1, n), rng.uniform(0, 360, n))]
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    # (a) host loop
    m = raft.Model(load_design("VolturnUS-S_farm"))
    state = ([(ln.HF, ln.VF) for ln in m.ms.lines], [p.r.copy() for p in m.ms.points])
    Xh = np.zeros([n, 12])
    t0 = time.perf_counter()
    evals = 0
    for i, c in enumerate(cases):
        for ln, (hf, vf) in zip(m.ms.lines, state[0]):
            ln.HF, ln.VF = hf, vf
        for p, r in zip(m.ms.points, state[1]):
            p.r = r.copy()
        Xh[i] = m.solveStatics(dict(c))
        evals += len(m.Xs2)
        m.ms.coupled_stiffness_analytic()
        m.ms.coupled_stiffness_fd(tensions=True)
    t_host = time.perf_counter() - t0
    say(f"(a) host loop, {n} cases: {t_host:.3f} s ({t_host / n * 1e3:.2f} ms per case, {evals / n:.2f} Newton "
        f"evaluations per case)")

    # (b) batched, whole call
    mb = raft.Model(load_design("VolturnUS-S_farm"))
    for _ in range(2):                                    # warm-up: code objects, allocator, the device records
        sb = mb.solveStaticsArrayBatch(cases)
    torch.cuda.synchronize()
    walls = []
    for _ in range(5):
        t0 = time.perf_counter()
        sb = mb.solveStaticsArrayBatch(cases)
        torch.cuda.synchronize()
        walls.append(time.perf_counter() - t0)
    walls = np.array(walls)
    assert not sb["status"].any()
    say(f"(b) solveStaticsArrayBatch wall, {n} cases: median {np.median(walls) * 1e3:.2f} ms (min {walls.min() * 1e3:.2f}, "
        f"max {walls.max() * 1e3:.2f}; host F_env, uploads, 2 launches, downloads)")
    rec, subs, X_ref, K_hs, F_const, warm0, free0 = mb._statics_array_inputs(cases)
    dm = DeviceArrayMooring([rec], mb.device)
    f64 = dict(dtype=torch.float64, device=dm.device)
    rep = lambda a: torch.tensor(np.tile(a, (n,) + (1,) * a.ndim), **f64)   # noqa: E731
    Xr, Kh, w0, f0, Fc = rep(X_ref), rep(K_hs), rep(warm0), rep(free0), torch.tensor(F_const, **f64)
    ev = []
    for r in range(15):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        sol = dm.solve_statics(Xr, Kh, Fc, w0, f0)
        dm.eval(sol["X"].view(n, 2, 6), sol["warm"], sol["free"], jacobian=True)
        b.record()
        b.synchronize()
        if r >= 5:
            ev.append(a.elapsed_time(b))
    ev = np.array(ev)
    say(f"(b) the two launches, HIP events: median {np.median(ev) * 1e3:.1f} us (min {ev.min() * 1e3:.1f}, max "
        f"{ev.max() * 1e3:.1f}; includes the output allocations between them)")
    say(f"ratio host loop / batched wall: {t_host / np.median(walls):.1f}x; host loop / launches: "
        f"{t_host / (np.median(ev) * 1e-3):.0f}x")
    say(f"max |X_batch - X_host| {np.abs(sb['X'] - Xh).max():.2e} m")
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 64, sys.argv[2] if len(sys.argv) > 2 else None)
