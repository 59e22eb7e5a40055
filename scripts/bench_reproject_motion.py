#!/usr/bin/env python3
"""Device time of flx_reproject across a pose of an object, and of flx_gbuffer with the object plane.

    python scripts/bench_reproject_motion.py OUTDIR [--calls 100] [--warmup 10] [--width 1920] [--height 1080]

scripts/bench_reproject.py's protocol (the kitchen stand-in of bench.build_workload, a 32 spp history written through flx_write_pixels, moments
on, the library's per-call events at flx_profile level 1, 100 calls after 10 warm-up calls, every measurement in a child process of its own
under its own time limit), four times:
  reproject_plain    option "motion_history" off, the camera moved by 0.05: the parent's flx_reproject on the same box (k_reproject)
  reproject_motion   the option on, scripts/bench_pose.py's object (about an eighth of the triangles) rotated by 0.02 rad between the capture and
                     the call, the same camera move: k_reproject_motion
  gbuffer_plain / gbuffer_objects   flx_gbuffer without and with the object plane
Writes OUTDIR/bench_reproject_motion.json with the byte model beside the measurements.  Nothing here is imported by the product or the tests;
bench.py's measurement is not involved.

Byte model of the motion-aware call (an ESTIMATE, not measured): DESIGN.md 4.3.3's ~130 unique bytes per pixel (current G 32 B, previous G
32 B, history 16 + 16 B, output 32 B) plus 4 B for the pixel's object id and 16 B for its four taps', at 6.3 TB/s achievable HBM bandwidth."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
BYTES_PER_PIXEL_PLAIN = 130
BYTES_PER_PIXEL_MOTION = 130 + 4 + 16
HBM_BYTES_PER_S = 6.3e12
KINDS = ("reproject_plain", "reproject_motion", "gbuffer_plain", "gbuffer_objects")


def child(a):
    import numpy as np
    import bench
    from bench_pose import rotation_about
    from bench_update_subset import box_subset
    from fluctus_amd.device import HipContext, K_GBUFFER, K_REPROJECT, NO_OBJECT
    W, H = a.width, a.height
    d, p, _ = bench.build_workload(W, H, "kitchen")
    motion = a.kind in ("reproject_motion", "gbuffer_objects")
    g = HipContext(W * H)
    g.set_option("moments", 1)
    g.set_option("motion_history", int(motion))
    g.upload_scene(d)
    g.set_params(p)
    idx, _ = box_subset(d, 0.125)
    P = np.stack([np.stack([d.tris[v]["p"][k][idx] for k in "xyz"], 1) for v in ("v0", "v1", "v2")], 1).astype(np.float64)
    centre = 0.5 * (P.min((0, 1)) + P.max((0, 1)))
    omap = np.full(d.tris.size, NO_OBJECT, np.uint32)
    omap[idx] = 0
    g.objects_define(d.tris, omap, 1)
    ids = np.zeros(1, np.uint32)
    g.objects_pose(ids, rotation_about(centre, 0.0))
    out = {"kind": a.kind, "object_triangles": int(idx.size), "triangles": int(d.tris.size)}
    if a.kind.startswith("gbuffer"):
        call, kid = g.gbuffer, K_GBUFFER
    else:
        rng = np.random.default_rng(1)
        px = np.zeros((W * H, 4), np.float32)
        px[:, :3] = rng.uniform(0.0, 64.0, (W * H, 3)); px[:, 3] = 32.0
        g.write_pixels(0, px); g.write_pixels(7, px)
        g.gbuffer(); g.history_capture()
        if motion:
            g.objects_pose(ids, rotation_about(centre, 0.02))
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
    out.update(ms_per_call=ms / max(1, n), calls=int(n))
    if a.kind.startswith("gbuffer"):
        out["share_hit"] = float((g.gbuffer_read(0)[0][:, 3].copy().view(np.int32) >= 0).mean())
    else:
        out["share_with_history"] = float((g.read_pixels(0)[:, 3] > 0).mean())
    if motion:
        plane = g.gbuffer_objects_read(0)
        out["share_object_pixels"] = float((plane == 0).mean())
        if a.kind == "reproject_motion":
            out["share_object_pixels_with_history"] = float((g.read_pixels(0)[plane == 0, 3] > 0).mean()) if (plane == 0).any() else None
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("outdir")
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--limit", type=int, default=240, help="seconds per child process")
    ap.add_argument("--kind", choices=KINDS, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.kind:
        return child(a)
    out = {"width": a.width, "height": a.height, "scene": "kitchen (bench.build_workload)", "object": "bench_pose.py's: about an eighth of the triangles, rotated by 0.02 rad"}
    for k in KINDS:
        cmd = [sys.executable, os.path.abspath(__file__), a.outdir, "--kind", k, "--calls", str(a.calls), "--warmup", str(a.warmup),
               "--width", str(a.width), "--height", str(a.height)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=a.limit)
        if r.returncode != 0:
            sys.stdout.write(r.stdout)
            raise SystemExit(f"{k}: child exited with {r.returncode}")            # nothing more is started on the GPU
        out[k] = json.loads(r.stdout.strip().splitlines()[-1])
    npix = a.width * a.height
    for kind, b in (("reproject_plain", BYTES_PER_PIXEL_PLAIN), ("reproject_motion", BYTES_PER_PIXEL_MOTION)):
        model_ms = npix * b / HBM_BYTES_PER_S * 1e3
        out[kind]["model_ms"] = model_ms
        out[kind]["model"] = f"not measured: {b} B per pixel at {HBM_BYTES_PER_S / 1e12} TB/s"
        out[kind]["model_share_of_measured"] = model_ms / out[kind]["ms_per_call"] if out[kind]["ms_per_call"] else None
    os.makedirs(a.outdir, exist_ok=True)
    with open(os.path.join(a.outdir, "bench_reproject_motion.json"), "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
