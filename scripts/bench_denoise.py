#!/usr/bin/env python3
"""Device time of flx_denoise at 1920 x 1080 on synthetic inputs fed through flx_write_pixels.

    python scripts/bench_denoise.py OUTDIR [--iterations 5] [--calls 200] [--warmup 20] [--variance-guided]

--variance-guided times flx_denoise_variance_guided instead, with random luminance moments (which = 7), into
OUTDIR/bench_denoise_vg.json, with its own roof model: the 25 taps at VG_VALU_PER_TAP plus 9 prefilter taps at VG_VALU_PER_PREFILTER_TAP.

Warms up, then times `calls` calls with the library's per-kernel events (flx_profile level 1, FLX_K_DENOISE: one event pair around the whole
call) and writes OUTDIR/bench_denoise.json: ms per call, and the VALU-issue roof of the model below beside it.  Nothing here is imported by the
product or the tests; bench.py is not involved.

Roof model (an ESTIMATE, not measured): a pass costs 25 taps x VALU_PER_TAP wave64 instructions per pixel at 4 SIMD cycles each (the single-issue
pipe: expf_ is a chain of dependent multiplies, floor and a conversion), on 256 CUs x 4 SIMDs at 2.4 GHz = 39.3 T lane-ops/s."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

VALU_PER_TAP = 45           # model: ~20 for expf_, ~12 for the three squared differences, ~8 for the weight and the sums, bounds and validity
VG_VALU_PER_TAP = 48        # model (variance-guided): the above with lum + |dl| / den in place of |de|^2, plus the w^2 var sum
VG_VALU_PER_PREFILTER_TAP = 8   # model: bounds, validity, one weight product and two adds per 3 x 3 prefilter tap
LANE_OPS_PER_S = 256 * 4 * 64 / 4 * 2.4e9


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("outdir")
    ap.add_argument("--iterations", type=int, default=5)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--variance-guided", action="store_true", help="time flx_denoise_variance_guided (DESIGN.md 4.3.2) instead")
    a = ap.parse_args()
    import common
    import denoise_reference as R
    from fluctus_amd.device import HipContext
    W, H = a.width, a.height
    d = common.simple_scene()
    g = HipContext(W * H)
    g.set_option("denoiser", 1)
    if a.variance_guided:
        g.set_option("moments", 1)
    g.upload_scene(d)
    g.set_params(common.scene_params(d, W, H))
    px, alb, nrm = R.random_inputs(W, H, 1)
    g.write_pixels(0, px); g.write_pixels(4, alb); g.write_pixels(5, nrm)
    call = g.denoise
    if a.variance_guided:
        import denoise_vg_reference as V
        g.write_pixels(7, V.random_inputs(W, H, 1)[3])
        call = g.denoise_variance_guided
    for _ in range(a.warmup):
        call(iterations=a.iterations)
    g.finish()
    g.profile_reset(); g.profile_enable(1)
    for _ in range(a.calls):
        call(iterations=a.iterations)
    g.finish(); g.profile_enable(0)
    ms, n = g.denoise_profile()
    per_call = ms / max(1, n)
    per_pass = 25 * VG_VALU_PER_TAP + 9 * VG_VALU_PER_PREFILTER_TAP if a.variance_guided else 25 * VALU_PER_TAP
    lane_ops = W * H * a.iterations * per_pass
    roof_ms = lane_ops / LANE_OPS_PER_S * 1e3
    out = {"filter": "variance_guided" if a.variance_guided else "guided", "width": W, "height": H, "iterations": a.iterations, "calls": int(n), "ms_per_call": per_call,
           "valu_roof_ms_model": roof_ms, "share_of_valu_roof": roof_ms / per_call if per_call else None,
           "roof_model": (f"not measured: ({VG_VALU_PER_TAP} VALU/tap x 25 taps + {VG_VALU_PER_PREFILTER_TAP} VALU/tap x 9 prefilter taps)"
                          if a.variance_guided else f"not measured: {VALU_PER_TAP} VALU/tap x 25 taps") +
                         f" x {a.iterations} passes per pixel, 4 cycles per wave64 instruction, "
                         "256 CUs x 4 SIMDs x 2.4 GHz"}
    os.makedirs(a.outdir, exist_ok=True)
    with open(os.path.join(a.outdir, "bench_denoise_vg.json" if a.variance_guided else "bench_denoise.json"), "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
