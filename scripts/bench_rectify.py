#!/usr/bin/env python3
"""Device time of flx_history_rectify.

    python scripts/bench_rectify.py OUTDIR [--calls 20] [--warmup 3] [--width 1920] [--height 1080]

Timed on the G-buffer of the kitchen stand-in (bench.py's headline workload: its scene, tree and camera, built by bench.build_workload) with a
32 spp history and 4 new samples per pixel written through flx_write_pixels, the new samples at half the history's brightness on the left half
of the image (so about half of the surface pixels shed history and are written) and noisy copies of it on the right.  Every call starts from
the same state: history written, flx_history_mark, new state written, then the call under the library's per-kernel events (flx_profile level
1, FLX_K_RECTIFY: one event pair around the two kernels).  radius 1, 3, 4, each with moments on and off, each configuration in a child process
of its own under its own time limit.  Writes OUTDIR/bench_rectify.json with the cost model beside the measurement.  Nothing here is imported by
the product or the tests; bench.py's measurement is not involved.

Cost model (an ESTIMATE, not measured): unique bytes per pixel at 6.3 TB/s achievable HBM bandwidth.  Prepare pass: A 16 + S 16 + G0 16 read,
record 16 written = 64 B.  Window pass: record 16 + G 32 + A 16 + S 16 read, lambda 4 written = 84 B; a pixel with lambda > 0 writes A and S
(32 B) and, with moments, reads and writes M and SM (64 B).  The halo's re-reads ((16 + 2 r)^2 / 256 of 48 B) are taken as L2 hits."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
HBM_BYTES_PER_S = 6.3e12


def model_bytes(share_written, moments):
    return 64 + 84 + share_written * (32 + (64 if moments else 0))


def child(a):
    import numpy as np
    import bench
    from fluctus_amd.device import HipContext, K_RECTIFY
    W, H = a.width, a.height
    N = W * H
    d, p, _ = bench.build_workload(W, H, "kitchen")
    g = HipContext(N)
    g.set_option("moments", a.moments)
    g.upload_scene(d)
    g.set_params(p)
    g.gbuffer()
    rng = np.random.default_rng(1)
    tex = rng.uniform(0.5, 1.5, N).astype(np.float32)
    S = np.zeros((N, 4), np.float32); S[:, :3] = (tex * 32.0)[:, None]; S[:, 3] = 32.0
    new = tex * rng.uniform(0.7, 1.3, N).astype(np.float32) * np.where(np.arange(N) % W < W // 2, 0.5, 1.0).astype(np.float32)
    A = S.copy(); A[:, :3] += (new * 4.0)[:, None]; A[:, 3] += 4.0
    SM = np.zeros((N, 4), np.float32); SM[:, 0] = tex * 32.0; SM[:, 1] = (tex * tex + 0.05) * 32.0; SM[:, 3] = 32.0
    M = SM.copy(); M[:, 0] += new * 4.0; M[:, 1] += new * new * 4.0; M[:, 3] += 4.0

    def call():
        g.write_pixels(0, S)
        if a.moments:
            g.write_pixels(7, SM)
        g.history_mark()
        g.write_pixels(0, A)
        if a.moments:
            g.write_pixels(7, M)
        g.history_rectify(radius=a.radius)

    for _ in range(a.warmup):
        call()
    g.finish()
    g.profile_reset(); g.profile_enable(1)
    for _ in range(a.calls):
        call()
    g.finish(); g.profile_enable(0)
    ms, n = g.kernel_profile(K_RECTIFY)
    lam = g.history_mark_read()[2]
    hit = g.gbuffer_read(0)[0][:, 3].copy().view(np.int32) >= 0
    print(json.dumps({"radius": a.radius, "moments": a.moments, "ms_per_call": ms / max(1, n), "calls": int(n),
                      "share_surface": float(hit.mean()), "share_written": float((lam > 0).mean()), "mean_lambda": float(lam.mean())}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("outdir")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--limit", type=int, default=240, help="seconds per configuration's child process")
    ap.add_argument("--radius", type=int, help=argparse.SUPPRESS)
    ap.add_argument("--moments", type=int, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.radius is not None:
        return child(a)
    out = {"width": a.width, "height": a.height, "scene": "kitchen (bench.build_workload)", "runs": []}
    for r in (1, 3, 4):
        for mom in (1, 0):
            cmd = [sys.executable, os.path.abspath(__file__), a.outdir, "--radius", str(r), "--moments", str(mom), "--calls", str(a.calls),
                   "--warmup", str(a.warmup), "--width", str(a.width), "--height", str(a.height)]
            res = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=a.limit)
            if res.returncode != 0:
                sys.stdout.write(res.stdout)
                raise SystemExit(f"radius {r}, moments {mom}: child exited with {res.returncode}")     # nothing more is started on the GPU
            run = json.loads(res.stdout.strip().splitlines()[-1])
            b = model_bytes(run["share_written"], mom)
            run["model_bytes_per_pixel"] = b
            run["model_ms"] = a.width * a.height * b / HBM_BYTES_PER_S * 1e3
            run["model"] = f"not measured: {b:.0f} B per pixel at {HBM_BYTES_PER_S / 1e12} TB/s"
            out["runs"].append(run)
    os.makedirs(a.outdir, exist_ok=True)
    with open(os.path.join(a.outdir, "bench_rectify.json"), "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
