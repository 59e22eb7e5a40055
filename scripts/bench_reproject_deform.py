#!/usr/bin/env python3
"""Device time of flx_reproject across a per-triangle move, of flx_gbuffer with the barycentric plane, and of the snapshot and the moved-flag
passes on their own.

    python scripts/bench_reproject_deform.py OUTDIR [--calls 100] [--warmup 10] [--width 1920] [--height 1080]

scripts/bench_reproject_motion.py's protocol (the kitchen stand-in of bench.build_workload, a 32 spp history written through flx_write_pixels,
moments on, the library's per-call events at flx_profile level 1, 100 calls after 10 warm-up calls, every measurement in a child process of its
own under its own time limit), six times:
  reproject_plain    option "deform_history" off, the camera moved by 0.05: the parent's flx_reproject on the same box (k_reproject)
  reproject_deform   the option on, scripts/bench_update_subset.py's box of about an eighth of the triangles displaced by 0.02 through
                     flx_update_triangles_subset between the capture and the call, the same camera move: k_moved_flags + k_reproject_deform
  gbuffer_plain / gbuffer_bary   flx_gbuffer without and with the barycentric plane
  snapshot           k_snapshot_positions alone (FLX_K_SNAPSHOT): gbuffer, capture, move -- once per call
  moved_flags        k_moved_flags alone (FLX_K_MOVED_FLAGS, as flx_deform_read launches it)
Writes OUTDIR/bench_reproject_deform.json with the byte model beside the measurements.  Nothing here is imported by the product or the tests;
bench.py's measurement is not involved.

Byte model (an ESTIMATE, written before anything was measured), at 6.3 TB/s achievable HBM bandwidth:
  k_reproject_deform  DESIGN.md 4.3.3's ~130 unique bytes per pixel (current G 32 B, previous G 32 B, history 16 + 16 B, output 32 B) plus 8 B
                      for the pixel's barycentrics and 1 B for its flag, 4 x (8 + 1) B for its four taps' -- neighbouring pixels share taps, so
                      about 8 + 1 unique -- and 96 B of positions for a pixel whose triangle moved (shared by the triangle's pixels: bounded by
                      96 B x moved triangles in view): ~148 B per pixel
  k_moved_flags       per triangle 3 x 16 B out of its 160-byte record -- three 64-byte sectors at least, 192 B fetched -- plus 48 B of snapshot
                      and 1 B written: ~241 B per triangle
  k_snapshot_positions   the same 192 B fetched, 48 B written: 240 B per triangle
  k_gbuffer<.., BARY>    8 B per pixel more than the 32 B it writes"""
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
BYTES_PER_PIXEL_DEFORM = 130 + 9 + 9
BYTES_PER_TRI_FLAGS = 192 + 48 + 1
BYTES_PER_TRI_SNAPSHOT = 192 + 48
HBM_BYTES_PER_S = 6.3e12
KINDS = ("reproject_plain", "reproject_deform", "gbuffer_plain", "gbuffer_bary", "snapshot", "moved_flags")
K_SNAPSHOT, K_MOVED_FLAGS = 14, 15           # FLX_K_SNAPSHOT / FLX_K_MOVED_FLAGS (include/fluctus_hip.h)


def child(a):
    import numpy as np
    import bench
    from bench_update_subset import box_subset
    from fluctus_amd.device import HipContext, K_GBUFFER, K_REPROJECT
    W, H = a.width, a.height
    d, p, _ = bench.build_workload(W, H, "kitchen")
    deform = a.kind not in ("reproject_plain", "gbuffer_plain")
    g = HipContext(W * H)
    g.set_option("moments", 1)
    g.set_option("deform_history", int(deform))
    g.upload_scene(d)
    g.set_params(p)
    idx, _ = box_subset(d, 0.125)
    idx = np.ascontiguousarray(idx, np.uint32)
    moved = d.tris[idx].copy()
    for v in ("v0", "v1", "v2"):
        moved[v]["p"]["x"] += np.float32(0.02)
    out = {"kind": a.kind, "moved_triangles": int(idx.size), "triangles": int(d.tris.size)}

    def history():
        rng = np.random.default_rng(1)
        px = np.zeros((W * H, 4), np.float32)
        px[:, :3] = rng.uniform(0.0, 64.0, (W * H, 3)); px[:, 3] = 32.0
        g.write_pixels(0, px); g.write_pixels(7, px)
        g.gbuffer(); g.history_capture()

    if a.kind.startswith("gbuffer"):
        call, kid = g.gbuffer, K_GBUFFER
    elif a.kind == "snapshot":
        history()
        rest = d.tris[idx].copy()
        state = {"k": 0}
        def call():                                          # every capture's first move snapshots; the moves alternate so that bytes change
            g.gbuffer(); g.history_capture()
            g.update_triangles_subset(moved if state["k"] % 2 == 0 else rest, idx)
            state["k"] += 1
        kid = K_SNAPSHOT
    else:
        history()
        if deform:
            g.update_triangles_subset(moved, idx)
        p["camera"]["pos"]["x"] += 0.05
        g.set_params(p); g.gbuffer()
        if a.kind == "moved_flags":
            call, kid = (lambda: g.deform_read(d.tris.size)), K_MOVED_FLAGS
        else:
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
    elif a.kind.startswith("reproject"):
        px = g.read_pixels(0)
        out["share_with_history"] = float((px[:, 3] > 0).mean())
        if deform:
            flags = g.deform_read(d.tris.size)[1]
            hit = g.gbuffer_read(0)[0][:, 3].copy().view(np.int32)
            on = (hit >= 0) & (g.gbuffer_bary_read(0)[:, 0] != -1.0) & flags[np.clip(hit, 0, None)]
            out["moved_flagged"] = int(flags.sum())
            out["share_moved_pixels"] = float(on.mean())
            out["share_moved_pixels_with_history"] = float((px[on, 3] > 0).mean()) if on.any() else None
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
    out = {"width": a.width, "height": a.height, "scene": "kitchen (bench.build_workload)",
           "move": "bench_update_subset.py's box: about an eighth of the triangles, displaced by 0.02 along x"}
    for k in KINDS:
        cmd = [sys.executable, os.path.abspath(__file__), a.outdir, "--kind", k, "--calls", str(a.calls), "--warmup", str(a.warmup),
               "--width", str(a.width), "--height", str(a.height)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=a.limit)
        if r.returncode != 0:
            sys.stdout.write(r.stdout)
            raise SystemExit(f"{k}: child exited with {r.returncode}")            # nothing more is started on the GPU
        out[k] = json.loads(r.stdout.strip().splitlines()[-1])
    npix, ntris = a.width * a.height, out["snapshot"]["triangles"]
    for kind, n, b, per in (("reproject_plain", npix, BYTES_PER_PIXEL_PLAIN, "pixel"), ("reproject_deform", npix, BYTES_PER_PIXEL_DEFORM, "pixel"),
                            ("snapshot", ntris, BYTES_PER_TRI_SNAPSHOT, "triangle"), ("moved_flags", ntris, BYTES_PER_TRI_FLAGS, "triangle")):
        model_ms = n * b / HBM_BYTES_PER_S * 1e3
        if kind == "reproject_deform":
            model_ms += ntris * BYTES_PER_TRI_FLAGS / HBM_BYTES_PER_S * 1e3           # the call runs the flag pass first
        out[kind]["model_ms"] = model_ms
        out[kind]["model"] = f"not measured: {b} B per {per} at {HBM_BYTES_PER_S / 1e12} TB/s" + (" plus the flag pass" if kind == "reproject_deform" else "")
        out[kind]["model_share_of_measured"] = model_ms / out[kind]["ms_per_call"] if out[kind]["ms_per_call"] else None
    os.makedirs(a.outdir, exist_ok=True)
    with open(os.path.join(a.outdir, "bench_reproject_deform.json"), "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
