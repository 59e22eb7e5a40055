"""CPU: the inputs of tests/test_gpu_splat.py are inputs on which the oracle reproduces ITSELF -- two oracle contexts with different thread counts, run
through the same calls, agree on counters and path state bit for bit and on every accumulator within common.fb_close -- and they have the shapes the
GPU tests rely on (every path terminating / none / a mix).  A device-vs-oracle difference there is then the device's."""
import numpy as np
import pytest
import common
import splat_cases as sc
from common import Q
from fluctus_amd import driver


def _oracles(case, n, denoiser=False):
    from oracle.binding import OracleContext
    d, p, env = case
    a, b = OracleContext(n, threads=8), OracleContext(n, threads=1)
    for c in (a, b):
        sc.setup(c, d, p, env, denoiser=denoiser)
    return a, b, int(p["width"]) * int(p["height"])


def _run(a, b, npix, iterations, moments=False):
    cnts, moms = [], [np.zeros((npix, 4)) if moments else None for _ in range(2)]
    for it in range(iterations):
        cs = [sc.oracle_iteration(c, npix, m) for c, m in zip((a, b), moms)]
        assert (cs[0] == cs[1]).all()
        for c in (a, b):
            c.wf_shadow(); c.clear_queues(); c.pixel_index_update(npix, int(cs[0][Q.RAYGEN]))
        cnts.append(cs[0])
    assert not common.state_diff(a.state_export(), b.state_export(), 0.0, 0.0)
    assert common.fb_close(a.read_pixels(0), b.read_pixels(0))
    if moments:
        assert common.fb_close(moms[0].astype(np.float32), moms[1].astype(np.float32))
    return cnts


@pytest.mark.parametrize("wh", [(4, 4), (3, 3)])
def test_sky_case_every_path_terminates(wh):
    a, b, npix = _oracles(sc.sky_case(*wh), 1000)
    cnts = _run(a, b, npix, 6)
    assert all(int(c[Q.RAYGEN]) == 1000 for c in cnts)
    px = a.read_pixels(0)
    assert int(px[:, 3].sum()) == 5000 and (px[:, 3] >= 5000 // npix - 5).all() and (px[:, :3].sum(1) > 0).all()


def test_box_case_no_path_terminates():
    a, b, npix = _oracles(sc.box_case(32, 32), 4096)
    cnts = _run(a, b, npix, 2)
    assert int(cnts[0][Q.RAYGEN]) == 4096 and int(cnts[1][Q.RAYGEN]) == 0
    assert not a.read_pixels(0).any()


@pytest.mark.parametrize("kind,n", [("kitchen", 4096), ("conference", 17 * 256)])
def test_mixed_cases(kind, n):
    a, b, npix = _oracles(sc.proc_case(kind, 32, 32), n, denoiser=True)
    cnts = _run(a, b, npix, 6, moments=True)
    assert any(0 < int(c[Q.RAYGEN]) < n for c in cnts)
    for which in (4, 5):
        fa, fb = a.read_pixels(which), b.read_pixels(which)
        assert common.fb_close(fa, fb) and fa[:, 3].sum() > 0
    assert a.read_pixels(0)[:, 3].sum() > 0


def test_first_frame_case():
    d, p, env = sc.proc_case("kitchen", 25, 23)
    a, b, npix = _oracles((d, p, env), 4096)
    ca, cb = driver.first_frame(a, p, npix), driver.first_frame(b, p, npix)
    assert (ca == cb).all() and common.fb_close(a.read_pixels(0), b.read_pixels(0))
    assert a.read_pixels(0)[:, 3].sum() > 0
