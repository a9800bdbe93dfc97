"""Time the batched analysis of a mooring currentMod 1 design: N cases on VolturnUS-S_test with currentMod = 1
(40 bins; current speed in (0, 1.5] m/s, heading U(0, 360) deg, one seeded sea state each):
  (a) the wall time per call of analyzeCasesBatch(statics=True, pose_device=True, line_current=True) (one warm-up,
      then the median and range of 5 calls);
  (b) the only path such a design has without line_current: one host solveStatics + solveDynamics per case, all N
      cases once, on one model (host code this feature does not touch).  The answers of (a) are compared with the
      host's on a fresh model for each of the first 8 cases: on a reused model the lines' warm starts carry over from
      case to case, which moves the host's answers at the catenary tolerance (1e-5);
  (c) the two statics launches alone, by HIP events on inputs already on the device (5 warm-up runs, then the
      median of 25): rh_statics_solve_current + rh_moor_eval_current with the cases' currents, against
      rh_statics_solve + rh_moor_eval on the same cases and inputs (what a currentMod 0 design launches).  The ratio is
      what current on the lines costs on the device.
usage: line_current_time.py [N] [out.txt] [pose_chunk]"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "raft-teststuff_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main(n, out_path=None, pose_chunk=32):
    import torch
    import raft
    from conftest import load_design
    rng = np.random.default_rng(512)
    base = {"wind_speed": 0, "wind_heading": 0, "turbulence": 0, "turbine_status": "operating", "yaw_misalign": 0,
            "wave_spectrum": "JONSWAP"}
    cases = [dict(base, current_speed=float(u), current_heading=float(h), wave_period=float(tp), wave_height=float(hs),
                  wave_heading=float(wh))
             for u, h, tp, hs, wh in zip(1.5 * (1.0 - rng.uniform(0, 1, n)), rng.uniform(0, 360, n), rng.uniform(6, 14, n),
                                         rng.uniform(1, 6, n), rng.uniform(-180, 180, n))]
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def model():
        d = load_design("VolturnUS-S_test")
        d["mooring"]["currentMod"] = 1
        d["settings"].update(min_freq=0.01, max_freq=0.4)
        return raft.Model(d)

    # (a) the whole call
    m = model()
    assert m.nw == 40 and m.mooring_currentMod == 1
    walls = []
    for rep in range(6):
        t0 = time.perf_counter()
        res = m.analyzeCasesBatch([dict(c) for c in cases], statics=True, pose_chunk=pose_chunk, pose_device=True,
                                  line_current=True)
        torch.cuda.synchronize()
        if rep:                                            # (the first call warms up code objects and the allocator)
            walls.append(time.perf_counter() - t0)
    w = np.array(walls)
    say(f"    cases with a statics status: {int(np.count_nonzero(res['statics_status']))}, with a failed drag fixed point: "
        f"{int(np.count_nonzero(res['status'] < 0))}")
    say(f"(a) analyzeCasesBatch(statics=True, pose_device=True, line_current=True), {n} cases, pose_chunk {pose_chunk}: "
        f"median {np.median(w):.3f} s (min {w.min():.3f}, max {w.max():.3f}; {np.median(w) / n * 1e3:.3f} ms per case); "
        f"statics evaluations {res['statics_iters'].min()}..{res['statics_iters'].max()}")

    # (b) the host path, per case
    mh = model()
    fh = mh.fowtList[0]
    fh.calcBEM()
    mh.solveStatics(dict(cases[0]))
    mh.solveDynamics(dict(cases[0]))                       # warm-up
    raised = 0
    t0 = time.perf_counter()
    for i, c in enumerate(cases):
        try:
            mh.solveStatics(dict(c))
            mh.solveDynamics(dict(c))
        except (RuntimeError, ValueError) as e:            # (the host catenary gives up on some shapes in strong current)
            raised += 1
            print(f"    host case {i} raised {e!r}", flush=True)
            continue
        if i % 64 == 63:
            print(f"    host case {i + 1} / {n}: {time.perf_counter() - t0:.1f} s", flush=True)
    th = time.perf_counter() - t0
    err = 0.0
    for i in range(min(n, 8)):
        mf = model()
        mf.fowtList[0].calcBEM()
        mf.solveStatics(dict(cases[i]))
        Xi = mf.solveDynamics(dict(cases[i]))
        err = max(err, float(np.linalg.norm(res["Xi"][i] - Xi[0]) / np.linalg.norm(Xi[0])))
    say(f"(b) host solveStatics + solveDynamics per case, {n} cases: {th:.2f} s ({th / n * 1e3:.2f} ms per case); "
        f"ratio to (a): {th / np.median(w):.1f}x; cases the host raised on: {raised}; max normwise Xi residual of (a) "
        f"against fresh host models, first {min(n, 8)} cases: {err:.2e}")

    # (c) the two statics launches alone
    dm, X_ref, K_hs, F_const, warm0 = m._statics_batch_inputs([dict(c) for c in cases], current_device=True,
                                                                line_current=True)
    dev = dict(X_ref=dm.f64(np.tile(X_ref, (n, 1)), [n, 6]), K_hs=dm.f64(np.tile(K_hs, (n, 1, 1)), [n, 6, 6]),
               F_const=dm.f64(F_const, [n, 6]), warm0=dm.f64(np.tile(warm0, (n, 1, 1)), [n, dm.nl_max, 2]))
    cur = m._line_currents(cases)
    med = {}
    for name, current in (("rh_statics_solve + rh_moor_eval", None),
                          ("rh_statics_solve_current + rh_moor_eval_current", cur)):
        ev = []
        for r in range(30):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            sol = dm.solve_statics(dev["X_ref"], dev["K_hs"], dev["F_const"], dev["warm0"], current=current)
            out = dm.eval(sol["X"], warm=sol["warm"], jacobian=True, current=current)
            b.record()
            b.synchronize()
            if r >= 5:
                ev.append(a.elapsed_time(b))
        ev = np.array(ev)
        med[name] = np.median(ev)
        say(f"(c) {name}, {n} cases, HIP events: median {np.median(ev) * 1e3:.1f} us (min {ev.min() * 1e3:.1f}, max "
            f"{ev.max() * 1e3:.1f}; evaluations {int(sol['iters'].min())}..{int(sol['iters'].max())}; includes the "
            f"current's upload and the output allocations)")
    a, b = med.values()
    say(f"    current on the lines costs {b / a:.2f}x on the device ({(b - a) * 1e3:.1f} us per {n} cases)")
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as fh_:
            fh_.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 512, sys.argv[2] if len(sys.argv) > 2 else None,
         int(sys.argv[3]) if len(sys.argv) > 3 else 32)
