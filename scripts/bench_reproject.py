#!/usr/bin/env python3
"""Device time of flx_gbuffer and flx_reproject.

    python scripts/bench_reproject.py OUTDIR [--calls 100] [--warmup 10] [--width 1920] [--height 1080]

flx_gbuffer is timed on the kitchen stand-in (bench.py's headline workload: its scene, tree and camera, built by bench.build_workload), flx_reproject on a G-buffer pair of that scene under two cameras a small move apart with a 32 spp history written through
flx_write_pixels, moments on.  Both with the library's per-kernel events (flx_profile level 1, FLX_K_GBUFFER / FLX_K_REPROJECT: one event
pair around each call), each kernel in a child process of its own under its own time limit.  Writes OUTDIR/bench_reproject.json with the
cost model of flx_reproject beside the measurement.  Nothing here is imported by the product or the tests; bench.py's measurement is not involved.

Cost model of flx_reproject (an ESTIMATE, not measured): ~130 unique bytes per pixel (current G 32 B, previous G 32 B, history 16 + 16 B,
output 32 B) at 6.3 TB/s achievable HBM bandwidth."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
BYTES_PER_PIXEL = 130
HBM_BYTES_PER_S = 6.3e12


def child(a):
    import numpy as np
    import bench
    from fluctus_amd.device import HipContext, K_GBUFFER, K_REPROJECT
    W, H = a.width, a.height
    d, p, _ = bench.build_workload(W, H, "kitchen")
    g = HipContext(W * H)
    g.set_option("moments", 1)
    g.upload_scene(d)
    g.set_params(p)
    if a.kernel == "gbuffer":
        call, kid = g.gbuffer, K_GBUFFER
    else:
        rng = np.random.default_rng(1)
        px = np.zeros((W * H, 4), np.float32)
        px[:, :3] = rng.uniform(0.0, 64.0, (W * H, 3)); px[:, 3] = 32.0
        g.write_pixels(0, px); g.write_pixels(7, px)
        g.gbuffer(); g.history_capture()
        p["camera"]["pos"]["x"] += 0.05
        g.set_params(p); g.gbuffer()
        call, kid = g.reproject, K_REPROJECT
    for _ in range(a.warmup):
        call()
    g.finish()
    g.profile_reset(); g.profile_enable(1)
    for _ in range(a.calls):
        call()
    g.finish(); g.profile_enable(0)
    ms, n = g.kernel_profile(kid)
    hits = None
    if a.kernel == "gbuffer":
        hits = float((g.gbuffer_read(0)[0][:, 3].copy().view(np.int32) >= 0).mean())
    else:
        hits = float((g.read_pixels(0)[:, 3] > 0).mean())
    print(json.dumps({"kernel": a.kernel, "ms_per_call": ms / max(1, n), "calls": int(n), "share_hit_or_with_history": hits}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("outdir")
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--limit", type=int, default=240, help="seconds per kernel's child process")
    ap.add_argument("--kernel", choices=["gbuffer", "reproject"], help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.kernel:
        return child(a)
    out = {"width": a.width, "height": a.height, "scene": "kitchen (bench.build_workload)"}
    for k in ("gbuffer", "reproject"):
        cmd = [sys.executable, os.path.abspath(__file__), a.outdir, "--kernel", k, "--calls", str(a.calls), "--warmup", str(a.warmup),
               "--width", str(a.width), "--height", str(a.height)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=a.limit)
        if r.returncode != 0:
            sys.stdout.write(r.stdout)
            raise SystemExit(f"{k}: child exited with {r.returncode}")            # nothing more is started on the GPU
        out[k] = json.loads(r.stdout.strip().splitlines()[-1])
    model_ms = a.width * a.height * BYTES_PER_PIXEL / HBM_BYTES_PER_S * 1e3
    out["reproject_model_ms"] = model_ms
    out["reproject_model"] = f"not measured: {BYTES_PER_PIXEL} B per pixel at {HBM_BYTES_PER_S / 1e12} TB/s"
    out["reproject_share_of_model"] = model_ms / out["reproject"]["ms_per_call"] if out["reproject"]["ms_per_call"] else None
    os.makedirs(a.outdir, exist_ok=True)
    with open(os.path.join(a.outdir, "bench_reproject.json"), "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
