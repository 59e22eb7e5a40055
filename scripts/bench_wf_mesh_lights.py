#!/usr/bin/env python3
"""What emissive triangles cost as lights of the WAVEFRONT integrator (option "mesh_lights_wavefront").

    python scripts/bench_wf_mesh_lights.py OUTDIR [--scene kitchen] [--lamps 4000] [--steps 60] [--repeats 5] [--passes 8]

The room is scripts/bench_mesh_lights.py's: bench.py's stand-in scene in which the `--lamps` triangles nearest the ceiling get an emissive copy
of their material, at the scene's bench resolution and bounce count, no other light.  In a child process under its own time limit, per
configuration: settle from a reset (2 x maxBounces + 2 iterations), then `--repeats` windows of `--steps` iterations of bench.py's loop (logic,
raygen, materials, extend, shadow, end of iteration), each window ending in flx_finish; ms per iteration and Mrays/s (extension + shadow queue
lengths over the window's time) as the median of the windows, with the smallest and the largest beside it.  The configurations alternate
inside every repeat, so a drift of the box hits them alike:
  wf_on        both options on: the MESH instance of the plain logic pass and the unfused chain
  wf_off_fuse0 the options off under "fuse" 0: the same unfused chain without the MESH instance -- the difference prices that instance
  wf_off_fuse1 the options off under "fuse" 1: the shipped fused chain -- what a fused MESH instance could regain (the lamps are dark in both
               "off" rows: they show the cost of the chain, not the same image)
  mk_pass      one microkernel sample pass with "mesh_lights" on, beside them (another integrator: one sample per pixel per pass)
Writes OUTDIR/bench_wf_mesh_lights.json.  Nothing here is imported by the product or the tests; bench.py's measurement is not involved."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def child(a):
    import numpy as np
    import bench
    from fluctus_amd import driver, wire
    from fluctus_amd.device import HipContext
    d, p, _ = bench.build_workload(None, None, a.scene)
    y = (d.tris["v0"]["p"]["y"] + d.tris["v1"]["p"]["y"] + d.tris["v2"]["p"]["y"]) / 3.0
    lamps = np.sort(np.argsort(-y, kind="stable")[:a.lamps]).astype(np.uint32)
    uniq, inv = np.unique(d.tris["matId"][lamps], return_inverse=True)
    extra = d.materials[uniq].copy()
    for k in "xyz":
        extra["Ke"][k] = 10.0
    d.tris["matId"][lamps] = d.materials.size + inv
    d.materials = np.concatenate([d.materials, extra]).astype(wire.MATERIAL)
    p["useAreaLight"], p["useEnvMap"] = 0, 0
    W, H = int(p["width"]), int(p["height"])
    settle = 2 * int(p["maxBounces"]) + 2
    configs = {"wf_on": dict(mesh_lights=1, mesh_lights_wavefront=1, fuse=1), "wf_off_fuse0": dict(mesh_lights=0, mesh_lights_wavefront=0, fuse=0),
               "wf_off_fuse1": dict(mesh_lights=0, mesh_lights_wavefront=0, fuse=1)}
    ctxs = {}
    for name, opt in configs.items():
        g = HipContext(a.num_tasks)
        for k, v in opt.items():
            g.set_option(k, v)
        g.upload_scene(d)
        g.set_params(p)
        driver.reset_renderer(g)
        for _ in range(settle):
            bench.step_async(g)
        g.finish()
        g.counter_totals(reset=True)
        ctxs[name] = g
    assert ctxs["wf_on"].mesh_lights_read()[0].size == lamps.size
    ms = {k: [] for k in configs}
    mrays = {k: [] for k in configs}
    for _ in range(a.repeats):
        for name, g in ctxs.items():
            g.finish()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                bench.step_async(g)
            g.finish()
            dt = time.perf_counter() - t0
            tot = g.counter_totals(reset=True)
            ms[name].append(dt / a.steps * 1e3)
            mrays[name].append((float(tot[1]) + float(tot[2])) / dt / 1e6)
    out = {"scene": a.scene, "triangles": int(d.tris.size), "lamps": int(lamps.size), "width": W, "height": H, "maxBounces": int(p["maxBounces"]),
           "num_tasks": a.num_tasks, "steps": a.steps, "repeats": a.repeats, "settle_iterations": settle}
    for name in configs:
        out[name] = {"ms_per_iteration": float(np.median(ms[name])), "ms_min": float(min(ms[name])), "ms_max": float(max(ms[name])),
                     "Mrays_s": float(np.median(mrays[name])), "Mrays_s_min": float(min(mrays[name])), "Mrays_s_max": float(max(mrays[name]))}
        ctxs[name].close()
    # the microkernel sample pass beside them: one sample per pixel per pass
    g = HipContext(W * H)
    g.set_option("mesh_lights", 1)
    g.upload_scene(d)
    q = p.copy(); q["useRoulette"] = 0
    g.set_params(q)
    g.mk_reset()
    for _ in range(2):
        driver.render_single_pass(g, q["maxBounces"])
    g.finish()
    g.mk_stats(reset=True)
    t = []
    for _ in range(a.passes):
        t0 = time.perf_counter()
        driver.render_single_pass(g, q["maxBounces"])
        g.finish()
        t.append((time.perf_counter() - t0) * 1e3)
    st = g.mk_stats()
    rays = float(st[0]) + float(st[1]) + float(st[2])
    out["mk_pass"] = {"ms_per_pass": float(np.median(t)), "ms_min": float(min(t)), "ms_max": float(max(t)), "Mrays_s": rays / (sum(t) * 1e-3) / 1e6, "passes": a.passes}
    g.close()
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("outdir")
    ap.add_argument("--scene", default="kitchen")
    ap.add_argument("--lamps", type=int, default=4000)
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--passes", type=int, default=8)
    ap.add_argument("--num-tasks", type=int, default=1 << 22)
    ap.add_argument("--limit", type=int, default=420, help="seconds for the child process")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)
    os.makedirs(a.outdir, exist_ok=True)
    cmd = [sys.executable, os.path.abspath(__file__), a.outdir, "--child", "--scene", a.scene, "--lamps", str(a.lamps), "--steps", str(a.steps),
           "--repeats", str(a.repeats), "--passes", str(a.passes), "--num-tasks", str(a.num_tasks)]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=a.limit)
    if r.returncode != 0:
        sys.stdout.write(r.stdout)
        raise SystemExit(f"child exited with {r.returncode}")
    out = {"what": "wall clock: emissive triangles as lights of the wavefront integrator on bench.py's stand-in room (DESIGN.md 4.2.3)",
           "result": json.loads(r.stdout.strip().splitlines()[-1])}
    with open(os.path.join(a.outdir, "bench_wf_mesh_lights.json"), "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
