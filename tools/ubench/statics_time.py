"""Time the mean-offset statics of N cases on VolturnUS-S_test (current speed U(0, 1) m/s, heading
U(0, 360) deg, seeded):
  (a) the host path: a Python loop of Model.solveStatics plus the central-difference tension
      Jacobian MooringSystem.coupled_stiffness_fd(tensions=True) at each offset pose;
  (b) Model.solveStaticsBatch: the wall time of the whole call (host F_env of every case, uploads,
      two launches, downloads) and the HIP-event time of the two launches alone (rh_statics_solve,
      rh_moor_eval with the Jacobian) on inputs already on the device.
Warm-up calls first; medians over the repeats, with the spread.  usage: statics_time.py [N] [out.txt]"""
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
    rng = np.random.default_rng(512)
    base = {"wind_speed": 0, "wind_heading": 0, "turbulence": 0, "turbine_status": "operating", "yaw_misalign": 0,
            "wave_spectrum": "JONSWAP", "wave_period": 0, "wave_height": 0, "wave_heading": 0}
    cases = [dict(base, current_speed=float(u), current_heading=float(h))
             for u, h in zip(rng.uniform(0, 1, n), rng.uniform(0, 360, n))]
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    # (a) host loop
    m = raft.Model(load_design("VolturnUS-S_test"))
    ms = m.fowtList[0].ms
    Xh = np.zeros([n, 6])
    for c in cases[:3]:                                   # warm-up
        m.solveStatics(dict(c))
        ms.coupled_stiffness_fd(tensions=True)
    t0 = time.perf_counter()
    evals = 0
    for i, c in enumerate(cases):
        Xh[i] = m.solveStatics(dict(c))
        evals += len(m.Xs2)
        ms.coupled_stiffness_fd(tensions=True)
    t_host = time.perf_counter() - t0
    say(f"(a) host loop, {n} cases: {t_host:.3f} s ({t_host / n * 1e3:.2f} ms per case, {evals / n:.2f} Newton "
        f"evaluations per case)")

    # (b) batched, whole call
    mb = raft.Model(load_design("VolturnUS-S_test"))
    for _ in range(3):                                    # warm-up: code objects, allocator, the device system
        sb = mb.solveStaticsBatch(cases)
    torch.cuda.synchronize()
    walls = []
    for _ in range(10):
        t0 = time.perf_counter()
        sb = mb.solveStaticsBatch(cases)
        torch.cuda.synchronize()
        walls.append(time.perf_counter() - t0)
    walls = np.array(walls)
    assert not sb["status"].any()
    say(f"(b) solveStaticsBatch wall, {n} cases: median {np.median(walls) * 1e3:.2f} ms (min {walls.min() * 1e3:.2f}, "
        f"max {walls.max() * 1e3:.2f}; host F_env, uploads, 2 launches, downloads)")
    # the two launches alone
    dm, X_ref, K_hs, F_const, warm0 = mb._statics_batch_inputs(cases)
    f64 = dict(dtype=torch.float64, device=dm.device)
    Xr = torch.tensor(np.tile(X_ref, (n, 1)), **f64)
    Kh = torch.tensor(np.tile(K_hs, (n, 1, 1)), **f64)
    Fc = torch.tensor(F_const, **f64)
    w0 = torch.tensor(np.tile(warm0, (n, 1, 1)), **f64)
    ev = []
    for r in range(25):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        sol = dm.solve_statics(Xr, Kh, Fc, w0)
        dm.eval(sol["X"], warm=sol["warm"], jacobian=True)
        b.record()
        b.synchronize()
        if r >= 5:
            ev.append(a.elapsed_time(b))
    ev = np.array(ev)
    say(f"(b) the two launches, HIP events: median {np.median(ev) * 1e3:.1f} us (min {ev.min() * 1e3:.1f}, max "
        f"{ev.max() * 1e3:.1f}; includes the output allocations between them)")
    say(f"ratio host loop / batched wall: {t_host / np.median(walls):.0f}x; host loop / launches: "
        f"{t_host / (np.median(ev) * 1e-3):.0f}x")
    # same answers: the host loop runs one case after another on ONE model (each solve starts from the
    # line state the previous case left), so it agrees with the batch at the catenary tolerance only
    say(f"max |X_batch - X_host| {np.abs(sb['X'] - Xh).max():.2e} m (host loop warm-started case to case)")
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 512, sys.argv[2] if len(sys.argv) > 2 else None)
