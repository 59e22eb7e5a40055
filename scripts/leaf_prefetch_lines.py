#!/usr/bin/env python3
"""What the leaf visit's early fetch of the first triangle (csrc/flx_trace4.h: wide_leaf_visit) costs in 128-byte line requests.

    python scripts/leaf_prefetch_lines.py [--workload kitchen] [--num-tasks 1048576] [--settle 24] [--iterations 3]

A leaf block whose header + first triangle (80 bytes) reach into one 128-byte line more than its header alone (32 bytes) costs one more line
request per visit whose box test FAILS (a visit that passes reads the triangle anyway).  The share of such blocks comes from the leaf offsets of
the tree (host); the share of failing visits from the host emulation of the device's traversal (tests/wide_analysis.cpp: leaf visits and leaf
boxes passed, on the product's own tree builder) over the steady-state extension and shadow rays of the workload, read from the device after
`--settle` iterations.  Prints both and their product per ray.  Needs a GPU; nothing here is imported by the product or the tests."""
import argparse
import ctypes as C
import os
import sys
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="kitchen"); ap.add_argument("--num-tasks", type=int, default=1 << 20)
    ap.add_argument("--settle", type=int, default=24); ap.add_argument("--iterations", type=int, default=3)
    a = ap.parse_args()
    import bench
    import conftest
    from common import COL, Q
    from fluctus_amd import driver
    from fluctus_amd.device import HipContext
    d, p, env = bench.build_workload(name=a.workload)
    npr = d.nodes["nPrims"].astype(np.int64); cnt = npr[npr > 0]
    off = 5 + np.concatenate([[0], np.cumsum(2 + 3 * cnt)[:-1]])            # flx_wide.h: the dummy leaf first, then one block per leaf in node order
    b0 = off * 16
    lines = lambda nbytes: (b0 + nbytes - 1) // 128 - b0 // 128 + 1
    extra = float((lines(80) > lines(32)).mean())
    print(f"{a.workload}: {cnt.size} leaf blocks, {cnt.mean():.2f} triangles per leaf; header straddles a line in {float((lines(32) == 2).mean()):.3f}; "
          f"header + first triangle touch one line more than the header in {extra:.3f} of the blocks")
    L = C.CDLL(conftest.build_wide_analysis()); L.fh_analysis_last_error.restype = C.c_char_p
    g = HipContext(a.num_tasks)
    g.upload_scene(d); g.upload_envmap(env); g.set_params(p); driver.reset_renderer(g)
    npix = int(p["width"]) * int(p["height"])
    for _ in range(a.settle):
        driver.benchmark_iteration(g, npix)
    tot = {"closest hit": np.zeros(5), "any hit": np.zeros(5)}
    for _ in range(a.iterations):
        g.wf_logic(False); g.wf_raygen(); g.wf_materials()
        c = g.get_counters(); g.finish(); c = np.array(c, copy=True)
        st = g.state_export()
        for name, q, o, dcol, mode in (("closest hit", Q.EXTENSION, COL.ORIG, COL.DIR, 0), ("any hit", Q.SHADOW, COL.SHADOW_ORIG, COL.SHADOW_DIR, 2 if p["useEnvMap"] and not p["useAreaLight"] else 1)):
            ids = g.queue_read(q)[:int(c[q])]
            r = np.zeros((ids.size, 8), np.float32)
            r[:, 0:3] = st[o:o + 3, ids].T; r[:, 4:7] = st[dcol:dcol + 3, ids].T
            r[:, 3] = 3.4028235e38 if mode == 0 else st[COL.SHADOW_LEN, ids]
            out = np.zeros(8, np.float64)
            rc = L.fh_wide_visits(d.nodes.ctypes.data_as(C.c_void_p), C.c_uint64(d.nodes.size), d.tris.ctypes.data_as(C.c_void_p), C.c_uint64(d.tris.size),
                                  d.indices.ctypes.data_as(C.c_void_p), C.c_uint64(d.indices.size), r.ctypes.data_as(C.c_void_p), C.c_uint64(ids.size), mode, out.ctypes.data_as(C.c_void_p))
            assert rc == 0, L.fh_analysis_last_error()
            tot[name] += np.array([ids.size, out[0], out[1], out[2], out[3]])
        g.wf_extend(); g.wf_shadow(); g.clear_queues(); g.finish()
        g.pixel_index_update(npix, int(c[0]))
    for name, (n, nv, lv, lp, tt) in tot.items():
        fail = 1.0 - lp / lv
        print(f"{name}: {int(n)} rays, per ray {nv / n:.2f} node visits, {lv / n:.3f} leaf visits of which {lp / n:.3f} pass the box test (fail rate {fail:.3f}), {tt / n:.2f} triangle tests; "
              f"line requests added by the early fetch = leaf visits x fail rate x {extra:.3f} = {lv / n * fail * extra:.4f} per ray, against {nv / n + lv / n:.2f} node and header requests")


if __name__ == "__main__":
    main()
