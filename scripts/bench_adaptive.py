#!/usr/bin/env python3
"""Device time of flx_mk_adaptive_update and of a microkernel sample pass over a list of active pixels: the kitchen stand-in
of bench.py at 1920 x 1080, 8 bounces, one path per pixel.

    python scripts/bench_adaptive.py OUTDIR [--calls 100] [--warmup 10] [--only unlisted]

Timed with HIP events on the context's stream (torch.cuda events on flx_stream), one pair around every call; writes OUTDIR/bench_adaptive.json:
  update        flx_mk_adaptive_update (classify + scan + scatter + the 4-byte read-back) on the moments of a 4-spp render, beside the byte model
  unlisted      one full sample pass over every pixel, no list (the path renderSingle takes; the same on the parent commit: --only unlisted)
  identity      the same pass through the list of all pixels
  clustered_X / scattered_X   a pass at X = 50 / 10 / 1 % active pixels: one contiguous run of rows / every k-th pixel
Every entry: median, min and max milliseconds over the calls.  Nothing here is imported by the product or the tests; bench.py is only asked
for its workload.

Byte model of the update, written down before measuring: 16 B of moments read per pixel (the neighbour rows come from L2), 1 B of flags
written and read again, 4 B per listed pixel; at 1080p with a quarter of the pixels listed 39 MB, 7.5 us at 5.2 TB/s -- the call is expected
to be bound by its three launches and the blocking read-back instead."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 5.2e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("outdir")
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--only", default=None, help="run only this entry (unlisted: also runs on a tree without the adaptive entry points)")
    a = ap.parse_args()
    import numpy as np
    import torch
    import bench
    from fluctus_amd import device, driver
    d, p, env = bench.build_workload()
    W, H = int(p["width"]), int(p["height"])
    N = W * H
    g = device.HipContext(N)
    g.set_option("moments", 1)
    g.upload_scene(d); g.upload_envmap(env)
    q = p.copy(); q["useRoulette"] = 0
    g.set_params(q); g.mk_reset()
    for _ in range(4):
        driver.render_single_pass(g, q["maxBounces"])
    g.finish()
    g.L.flx_stream.restype = __import__("ctypes").c_void_p
    stream = torch.cuda.ExternalStream(int(g.L.flx_stream(g.h)))

    def timed(fn):
        ms = []
        for i in range(a.warmup + a.calls):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream); fn(); e1.record(stream)
            g.finish(); e1.synchronize()
            if i >= a.warmup:
                ms.append(e0.elapsed_time(e1))
        ms = np.array(ms)
        return {"median_ms": float(np.median(ms)), "min_ms": float(ms.min()), "max_ms": float(ms.max()), "calls": int(ms.size)}

    def one_pass():
        driver.render_single_pass(g, q["maxBounces"])
    out = {"width": W, "height": H, "maxBounces": int(q["maxBounces"])}
    lists = {"unlisted": None}
    if a.only != "unlisted":
        lists["identity"] = np.arange(N, dtype=np.uint32)
        for pct in (50, 10, 1):
            rows = max(1, H * pct // 100)
            lists[f"clustered_{pct}"] = np.arange((H - rows) // 2 * W, ((H - rows) // 2 + rows) * W, dtype=np.uint32)
            lists[f"scattered_{pct}"] = np.arange(0, N, 100 // pct, dtype=np.uint32)
        if a.only in (None, "update"):
            n = g.mk_adaptive_update()
            model = N * 16 + 2 * N + 4 * n
            out["update"] = dict(timed(lambda: g.mk_adaptive_update()), active=n, model_bytes=model, model_us=model / HBM_BYTES_PER_S * 1e6)
            g.mk_adaptive_clear()
    for name, lst in lists.items():
        if a.only not in (None, name):
            continue
        if lst is None:
            if hasattr(g, "mk_adaptive_clear"):
                g.mk_adaptive_clear()
        else:
            g.mk_active_write(lst)
        out[name] = dict(timed(one_pass), active=N if lst is None else int(lst.size))
    if "unlisted" in out:
        for k, v in out.items():
            if isinstance(v, dict) and k not in ("unlisted", "update"):
                v["fraction_of_unlisted"] = v["median_ms"] / out["unlisted"]["median_ms"]
    os.makedirs(a.outdir, exist_ok=True)
    with open(os.path.join(a.outdir, "bench_adaptive.json"), "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
