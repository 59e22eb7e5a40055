#!/usr/bin/env python3
"""Cost of flx_update_triangles against the rebuild it replaces, and what the refitted tree costs to traverse.

    python scripts/bench_refit.py OUTDIR [--scenes kitchen conference courtyard-1440p] [--calls 20] [--warmup 3] [--iters 6]

Per scene (bench.py's stand-ins: scene, SBVH and camera from bench.build_workload), in a child process of its own under its own time limit:
  update    ms per flx_update_triangles for a host source (wall clock around the call + flx_finish: it includes the PCIe copy and the blocking
            validation read) and for a device source (a torch tensor), and the device time of the passes alone (flx_profile level 1,
            FLX_K_REFIT) with the GB/s they achieve against their byte count
  rebuild   what it replaces, timed the same way in the same run: host.build_bvh + flx_upload_scene of the moved scene
  traverse  Mrays/s of flx_wf_extend / flx_wf_shadow (flx_profile level 2) over --iters benchmark iterations from the same camera and seeds, on
            the refitted tree against a tree rebuilt for the same triangles, for a mild (2 % of the extent) and a strong (30 %) sine deformation
Writes OUTDIR/bench_refit.json.  Nothing here is imported by the product or the tests; bench.py's measurement is not involved.

Byte count of the passes (an ESTIMATE of the unique bytes, not measured): per triangle 160 read + 160 + 64 written (shade pass); per index-list
slot and per wide-leaf triangle 48 read + 48 gathered + 48 written; per wide leaf 32 + 32; per BNode record 64 + 64 and the child it reads 64;
per WNode 64 + 64 + 32 and 32 per child box."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def deformed(d, amount):
    """a copy of d (same tree) whose vertices moved by amount * extent * a sine field of their position"""
    import copy
    import numpy as np
    m = copy.copy(d)
    m.tris, m.nodes = d.tris.copy(), d.nodes.copy()
    P = np.stack([np.stack([d.tris[v]["p"][k] for k in "xyz"], 1) for v in ("v0", "v1", "v2")], 1).astype(np.float64)
    lo = P.min((0, 1)); ext = float((P.max((0, 1)) - lo).max())
    u = (P - lo) / ext
    f = np.stack([np.sin(5.0 * u[..., 1] + 1.0), np.sin(4.0 * u[..., 2] + 2.0), np.sin(6.0 * u[..., 0] + 3.0)], -1)
    P2 = np.float32(P + amount * ext * f)
    for i, v in enumerate(("v0", "v1", "v2")):
        for j, k in enumerate("xyz"):
            m.tris[v]["p"][k] = P2[:, i, j]
    return m


def pass_bytes(info, ntris, nidx):
    return (ntris * (160 + 160 + 64) + 2 * nidx * (48 + 48 + 48) + info["wide_nodes"] * (64 + 64 + 32 + 4 * 32) +
            info["binary_records"] * (64 + 64 + 64) + (info["wide_leaf_f4"] - 5 - 3 * nidx) // 2 * 64)


def traverse(g, d, p, env, iters):
    """Mrays/s of the two traversal kernels over `iters` benchmark iterations from a reset"""
    import numpy as np
    from fluctus_amd import driver
    g.set_params(p)
    if env is not None:
        g.upload_envmap(env)
    driver.reset_renderer(g)
    g.profile_reset(); g.profile_enable(2)
    rays = np.zeros(2, np.float64)
    for _ in range(iters):
        c = driver.benchmark_iteration(g, int(p["width"]) * int(p["height"]))
        rays += (float(c[1]), float(c[2]))              # extension, shadow queue lengths
    g.finish(); g.profile_enable(0)
    prof = g.profile_get()
    return {"extend_mrays_s": rays[0] / max(prof["extend"][0], 1e-9) / 1e3, "shadow_mrays_s": rays[1] / max(prof["shadow"][0], 1e-9) / 1e3}


def child(a):
    import torch
    import numpy as np
    import bench
    from fluctus_amd import host
    from fluctus_amd.device import HipContext, K_REFIT
    name = a.scene
    d, p, env = bench.build_workload(None, None, name)
    n = 1 << 20
    g = HipContext(n)
    g.upload_scene(d)
    info = g.scene_info()
    out = {"scene": name, "triangles": int(d.tris.size), "index_list": int(d.indices.size), "binary_records": info["binary_records"], "wide_nodes": info["wide_nodes"]}
    mild, strong = deformed(d, 0.02), deformed(d, 0.30)
    dev = torch.from_numpy(np.frombuffer(mild.tris.tobytes(), np.uint8).copy()).cuda()
    for src, on_dev, key in ((mild, False, "host_source"), (dev, True, "device_source")):
        for _ in range(a.warmup):
            g.update_triangles(src, on_device=on_dev)
        g.finish()
        g.profile_reset(); g.profile_enable(1)
        t0 = time.perf_counter()
        for _ in range(a.calls):
            g.update_triangles(src, on_device=on_dev)
            g.finish()
        wall = (time.perf_counter() - t0) / a.calls * 1e3
        g.profile_enable(0)
        ms, k = g.kernel_profile(K_REFIT)
        out[key] = {"ms_per_call_wall": wall, "ms_passes_device": ms / max(1, k), "calls": int(k)}
    nbytes = pass_bytes(info, d.tris.size, d.indices.size)
    out["pass_bytes_estimate"] = int(nbytes)
    out["passes_gb_s"] = nbytes / (out["device_source"]["ms_passes_device"] * 1e-3) / 1e9
    # what it replaces: rebuild on the CPU + upload, once per deformation (seconds)
    out["traverse"] = {}
    for label, m in (("mild_2pct", mild), ("strong_30pct", strong)):
        g.update_triangles(m); g.finish()
        host.refit_bvh(m)                                # world_radius of the moved scene for the parameters
        pm = p.copy(); pm["worldRadius"] = m.world_radius
        refit = traverse(g, m, pm, env, a.iters)
        t0 = time.perf_counter()
        host.build_bvh(m, "sbvh")
        t1 = time.perf_counter()
        g.upload_scene(m); g.finish()
        t2 = time.perf_counter()
        pm["worldRadius"] = m.world_radius
        rebuilt = traverse(g, m, pm, env, a.iters)
        out["traverse"][label] = {"refit": refit, "rebuilt": rebuilt, "rebuild_ms": {"build_bvh": (t1 - t0) * 1e3, "upload_scene": (t2 - t1) * 1e3}}
        g.upload_scene(d); g.finish()                    # back to the tree built for the rest pose
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("outdir")
    ap.add_argument("--scenes", nargs="+", default=["kitchen", "conference", "courtyard-1440p"])
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=6)
    ap.add_argument("--limit", type=int, default=420, help="seconds per scene's child process")
    ap.add_argument("--scene", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.scene:
        return child(a)
    out = {"schedule": "level-synchronous (the only one built)", "scenes": []}
    os.makedirs(a.outdir, exist_ok=True)
    for s in a.scenes:
        cmd = [sys.executable, os.path.abspath(__file__), a.outdir, "--scene", s, "--calls", str(a.calls), "--warmup", str(a.warmup), "--iters", str(a.iters)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=a.limit)
        if r.returncode != 0:
            sys.stdout.write(r.stdout)
            raise SystemExit(f"{s}: child exited with {r.returncode}")            # nothing more is started on the GPU
        out["scenes"].append(json.loads(r.stdout.strip().splitlines()[-1]))
        with open(os.path.join(a.outdir, "bench_refit.json"), "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
