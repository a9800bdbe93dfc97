"""Time analyzeCasesBatch(statics=True) of N cases on VolturnUS-S_test (40 bins; current speed U(0, 1) m/s,
heading U(0, 360) deg, one seeded sea state each) with the per-case host designs (pose_device=False) and
with the designs from the device (pose_device=True):
  (a) the wall time of the whole call, both forms interleaved in one process: one warm-up each, then the
      median and range of 5 calls each;
  (b) what remains of the pose_device=True call, by stage (host clocks around work that ends in a device
      synchronise): the statics' host inputs (_statics_batch_inputs: calcTurbineConstants and the case
      dictionaries of every case, one rh_current_loads launch), its two launches, and the chunks
      (rh_pose_designs, the count read-back, descriptors, rh_wave_tables_batch, rh_solve_cases);
  (c) the two new launches alone, by HIP events, on inputs already on the device.
usage: pose_time.py [N] [out.txt] [pose_chunk]"""
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
             for u, h, tp, hs, wh in zip(rng.uniform(0, 1, n), rng.uniform(0, 360, n), rng.uniform(6, 14, n),
                                         rng.uniform(1, 6, n), rng.uniform(-180, 180, n))]
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def model():
        d = load_design("VolturnUS-S_test")
        d["settings"].update(min_freq=0.01, max_freq=0.4)
        return raft.Model(d)

    def call(m, pose_device):
        t0 = time.perf_counter()
        r = m.analyzeCasesBatch([dict(c) for c in cases], statics=True, pose_chunk=pose_chunk, pose_device=pose_device)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, r

    # (a) whole calls, interleaved
    m0, m1 = model(), model()
    assert m0.nw == 40
    call(m0, False), call(m1, True)                        # warm-up: code objects, allocator, the device records
    walls = {False: [], True: []}
    for _ in range(5):
        for pd, m in ((False, m0), (True, m1)):
            t, r = call(m, pd)
            walls[pd].append(t)
            if pd:
                r1 = r
            else:
                r0 = r
    for pd in (False, True):
        w = np.array(walls[pd])
        say(f"(a) analyzeCasesBatch(statics=True, pose_device={pd}), {n} cases, pose_chunk {pose_chunk}: median "
            f"{np.median(w):.3f} s (min {w.min():.3f}, max {w.max():.3f}; {np.median(w) / n * 1e3:.2f} ms per case)")
    say(f"    ratio of the medians: {np.median(walls[False]) / np.median(walls[True]):.2f}x")
    err = np.linalg.norm(r1["Xi"] - r0["Xi"], axis=(1, 2)) / np.linalg.norm(r0["Xi"], axis=(1, 2))
    say(f"    same answers: max normwise Xi residual {err.max():.2e}, iteration counts equal: "
        f"{bool(np.array_equal(r1['iters'], r0['iters']))}")

    # (b) the stages of the pose_device=True call
    f = m1.fowtList[0]
    seas = [m1._case_sea_states(c) for c in cases]
    reps = {k: [] for k in ("statics inputs (host)", "statics launches and downloads (the call minus its inputs)", "chunks")}
    for _ in range(3):
        t0 = time.perf_counter()
        dm, X_ref, K_hs, F_const, warm0 = m1._statics_batch_inputs([dict(c) for c in cases], current_device=True)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        sb = m1._solve_statics_batch([dict(c) for c in cases], None, False, None, current_device=True)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        m1._pose_device_chunks(f, cases, seas, sb, None, 0.01, ("psd", "std", "zeta", "B_drag"), pose_chunk)
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        reps["statics inputs (host)"].append(t1 - t0)
        reps["statics launches and downloads (the call minus its inputs)"].append((t2 - t1) - (t1 - t0))
        reps["chunks"].append(t3 - t2)
    for k, v in reps.items():
        say(f"(b) {k}: median {np.median(v) * 1e3:.1f} ms ({np.median(v) / n * 1e6:.0f} us per case)")
    t0 = time.perf_counter()
    for c in cases:
        f.calcTurbineConstants(dict(c), ptfm_pitch=0)
    say(f"(b)   of the statics inputs, calcTurbineConstants of every case: {(time.perf_counter() - t0) * 1e3:.1f} ms")

    # (c) the two new launches alone
    from raft.pose_device import pose_record
    rec = pose_record(f, m1.device)
    X = sb["X"].contiguous()
    U = [c["current_speed"] for c in cases]
    H = [c["current_heading"] for c in cases]
    for name, fn in (("rh_pose_designs + count read-back", lambda: rec.pose_tables(X)),
                     ("rh_current_loads", lambda: rec.current_loads(f.r6, U, H, f.depth, 0.0, f.shearExp_water,
                                                                    f.rho_water))):
        ev = []
        for r in range(25):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            if r >= 5:
                ev.append(a.elapsed_time(b))
        ev = np.array(ev)
        say(f"(c) {name}, {n} rows, HIP events: median {np.median(ev) * 1e3:.1f} us (min {ev.min() * 1e3:.1f}, max "
            f"{ev.max() * 1e3:.1f}; includes the call's uploads and output allocations)")
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 512, sys.argv[2] if len(sys.argv) > 2 else None,
         int(sys.argv[3]) if len(sys.argv) > 3 else 32)
