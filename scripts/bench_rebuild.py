#!/usr/bin/env python
"""Measurements behind DESIGN.md 4.10.1 (the rebuild policy): python scripts/bench_rebuild.py OUTDIR [--scenes kitchen conference] -> OUTDIR/bench_rebuild.json

  threshold   per scene and sine-field amplitude (0, 0.5, 2, 10, 30 % of the extent; scripts/bench_refit.py's field): the eight sums of
              flx_tree_cost on the refitted trees, the 4-wide cost ratio against the fresh tree, and the flx_wf_extend / flx_wf_shadow rates of the
              refitted tree against a tree rebuilt for the same pose -- what tells a caller which threshold to pass
  trigger     ms per flx_tree_cost (HIP events, FLX_K_TREE_COST; 100 calls after 10 warm-up calls) beside flx_update_triangles' device-source passes
  series      a sine field whose amplitude grows to 30 % over --frames frames on the procedural kitchen through Tracer::updateGeometry + update(),
              under the policies off / blocking / background at --threshold: mean and longest frame, rebuild count, rays/s of the last frames
One child process per scene (and one for the series), each under a time limit; a failed child ends the run.
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
AMPLITUDES = (0.0, 0.005, 0.02, 0.10, 0.30)


def child_scene(a):
    import torch
    import numpy as np
    import bench
    import bench_refit
    from fluctus_amd import host
    from fluctus_amd.device import HipContext, K_REFIT, K_TREE_COST, tree_cost_value
    d, p, env = bench.build_workload(None, None, a.scene)
    g = HipContext(1 << 20)
    g.upload_scene(d)
    fresh = g.tree_cost()
    out = {"scene": a.scene, "triangles": int(d.tris.size), "fresh": {"binary": fresh[0], "wide": fresh[1], "wide_cost": tree_cost_value(fresh[1])}, "amplitudes": []}
    # the trigger's cost beside the refit's
    dev = torch.from_numpy(np.frombuffer(d.tris.tobytes(), np.uint8).copy()).cuda()
    for _ in range(10):
        g.tree_cost(); g.update_triangles(dev, on_device=True)
    g.finish(); g.profile_reset(); g.profile_enable(1)
    t0 = time.perf_counter()
    for _ in range(100):
        g.tree_cost()
    wall = (time.perf_counter() - t0) / 100 * 1e3
    for _ in range(100):
        g.update_triangles(dev, on_device=True)
    g.finish(); g.profile_enable(0)
    (ms_c, n_c), (ms_r, n_r) = g.kernel_profile(K_TREE_COST), g.kernel_profile(K_REFIT)
    out["trigger"] = {"tree_cost_ms_device": ms_c / max(1, n_c), "tree_cost_ms_wall": wall, "refit_ms_device": ms_r / max(1, n_r), "calls": int(n_c)}
    for amp in AMPLITUDES:
        m = bench_refit.deformed(d, amp)
        g.upload_scene(d); g.update_triangles(m); g.finish()
        sums = g.tree_cost()
        host.refit_bvh(m)
        pm = p.copy(); pm["worldRadius"] = m.world_radius
        refit = bench_refit.traverse(g, m, pm, env, a.iters)
        host.build_bvh(m, "sbvh")
        g.upload_scene(m); g.finish()
        rebuilt_sums = g.tree_cost()
        pm["worldRadius"] = m.world_radius
        rebuilt = bench_refit.traverse(g, m, pm, env, a.iters)
        out["amplitudes"].append({"amplitude": amp, "binary": sums[0], "wide": sums[1],
                                  "wide_cost_ratio_vs_fresh": tree_cost_value(sums[1]) / tree_cost_value(fresh[1]),
                                  "wide_cost_ratio_vs_rebuilt": tree_cost_value(sums[1]) / tree_cost_value(rebuilt_sums[1]),
                                  "refit": refit, "rebuilt": rebuilt,
                                  "extend_rate_refit_over_rebuilt": refit["extend_mrays_s"] / rebuilt["extend_mrays_s"],
                                  "shadow_rate_refit_over_rebuilt": refit["shadow_mrays_s"] / rebuilt["shadow_mrays_s"]})
    print(json.dumps(out))


def child_series(a):
    import numpy as np
    import bench_refit
    from fluctus_amd import host
    from fluctus_amd.tracer import Tracer
    kind, ntris, seed = "kitchen", a.series_tris, 42
    d = host.generate_scene(kind, ntris, seed)
    d.nodes = np.zeros(0)                                   # (bench_refit.deformed copies the node array along)
    out = {"scene": f"proc:{kind}:{ntris}:{seed}", "frames": a.frames, "threshold": a.threshold, "modes": {}}
    W, H = 1280, 720
    for mode in ("off", "blocking", "background"):
        t = Tracer(W, H, 0, 1 << 20)
        t.init(W, H, f"proc:{kind}:{ntris}:{seed}")
        t.set_rebuild_policy(mode, None if mode == "off" else a.threshold)
        t.update()
        ms, ratios = [], []
        for f in range(a.frames):
            tris = bench_refit.deformed(d, 0.30 * (f + 1) / a.frames).tris       # (outside the timed frame)
            t0 = time.perf_counter()
            t.update_geometry(tris)
            t.update()
            ms.append((time.perf_counter() - t0) * 1e3)
            ratios.append(t.last_cost_ratio)
        t.wait_for_rebuild()
        before = t.stats().astype(np.float64)
        t0 = time.perf_counter()
        for _ in range(20):                                 # the rate at the last pose
            t.update()
        dt = time.perf_counter() - t0
        rays = (t.stats().astype(np.float64) - before)[:3].sum()
        out["modes"][mode] = {"mean_frame_ms": float(np.mean(ms)), "longest_frame_ms": float(np.max(ms)), "longest_frame": int(np.argmax(ms)),
                              "rebuilds": t.rebuild_count, "last_cost_ratio": None if ratios[-1] != ratios[-1] else ratios[-1], "final_mrays_s": rays / dt / 1e6}
        t.close()
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("outdir")
    ap.add_argument("--scenes", nargs="+", default=["kitchen", "conference"])
    ap.add_argument("--iters", type=int, default=6)
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--series-tris", type=int, default=60000)
    ap.add_argument("--threshold", type=float, default=1.3)
    ap.add_argument("--no-series", action="store_true")
    ap.add_argument("--limit", type=int, default=420, help="seconds per child process")
    ap.add_argument("--scene", help=argparse.SUPPRESS)
    ap.add_argument("--series", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.scene:
        return child_scene(a)
    if a.series:
        return child_series(a)
    out = {"scenes": [], "series": None}
    os.makedirs(a.outdir, exist_ok=True)
    common = ["--iters", str(a.iters), "--frames", str(a.frames), "--series-tris", str(a.series_tris), "--threshold", str(a.threshold)]
    jobs = [["--scene", s] for s in a.scenes] + ([] if a.no_series else [["--series"]])
    for job in jobs:
        cmd = [sys.executable, os.path.abspath(__file__), a.outdir] + job + common
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=a.limit)
        if r.returncode != 0:
            sys.stdout.write(r.stdout)
            raise SystemExit(f"{job}: child exited with {r.returncode}")            # nothing more is started on the GPU
        res = json.loads(r.stdout.strip().splitlines()[-1])
        if job[0] == "--series":
            out["series"] = res
        else:
            out["scenes"].append(res)
        with open(os.path.join(a.outdir, "bench_rebuild.json"), "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
