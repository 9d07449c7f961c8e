"""The numpy restatement of the clearance field and the smoother (tests/smoother_ref.py) on its
own, without a GPU: the properties the smoother promises, shown on the arithmetic that
tests/test_gpu_smooth.py then holds the device to, bit for bit.

The crafted cases live in a 64 x 64 map at 0.5 m whose grid frame equals the world frame
(goal (25.5, 16, 0) seen from a start on the same y: heading 0, goal cell (51, 32)).
"""
import math

import numpy as np

from tests import smoother_ref as sr

N, RES = 64, 0.5
THR = np.float32(math.log(0.75 / (1.0 - 0.75)))
FRAME = np.array([1.0, 0.0, 25.5, 16.0, 25.5, 16.0, RES, THR], np.float32)
GOAL, START = [25.5, 16.0, 0.0], [5.0, 16.0, 0.0]  # update_goal arguments that give FRAME
KAPPA = np.float32(math.tan(math.radians(30.0)) / 2.269)  # about the harness vehicle's largest curvature
FREE, OCC = np.float32(-2.0), np.float32(3.0)


def empty_map():
    return np.full((N, N), FREE, np.float32)


def wall_map():
    """A wall one cell thick: cells i = 20 (x = 10 m), j = 10 .. 50 (y = 5 .. 25 m)."""
    m = empty_map()
    m[20, 10:51] = OCC
    return m


def with_headings(xy):
    """(n, 3) float32 path, goal -> start: each heading is the direction of travel (decreasing i)."""
    xy = np.asarray(xy, np.float32)
    d = np.empty_like(xy)
    d[1:-1] = xy[:-2] - xy[2:]
    d[0], d[-1] = xy[0] - xy[1], xy[-2] - xy[-1]
    return np.column_stack([xy, np.arctan2(d[:, 1], d[:, 0])]).astype(np.float32)


def collinear(n=24):
    k = np.arange(n - 1, -1, -1, dtype=np.float32)
    return with_headings(np.column_stack([4.0 + 0.5 * k, 8.0 + 0.25 * k]))


def zigzag(n=30):
    k = np.arange(n - 1, -1, -1, dtype=np.float32)
    return with_headings(np.column_stack([4.0 + 0.5 * k, 12.0 + 0.2 * ((k.astype(int) % 2) * 2 - 1)]))


def wall_polyline():
    """Leaves x = 9 m, swings out to x = 10.5 m (one cell from the wall's cells at x = 10 m) for
    the wall's whole length, and comes back: its chord runs through the wall."""
    y = np.arange(29.0, 0.75, -0.5, dtype=np.float32)
    x = np.where((y >= 4.5) & (y <= 25.5), 10.5, np.where((y >= 4.0) & (y <= 26.0), 9.75, 9.0)).astype(np.float32)
    return with_headings(np.column_stack([x, y]))


def run(path, occ, **opts):
    d2 = sr.edt_brute(occ, THR)
    return sr.smooth_ref(path, np.zeros(len(path), np.float32), None, FRAME, occ, d2, KAPPA, **opts), d2


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_collinear_polyline_is_a_fixed_point():
    p = collinear()
    r, _ = run(p, empty_map())
    assert r["blend"] == 1.0 and r["status"] == 0
    assert np.array_equal(bits(r["path"]), bits(p))
    assert np.array_equal(bits(r["curvature"]), bits(np.zeros(len(p))))


def test_zigzag_gets_smoother_and_keeps_its_ends():
    p = zigzag()
    r, _ = run(p, empty_map())
    assert r["blend"] > 0
    assert sr.sum_second_diff2(r["path"]) < 0.5 * sr.sum_second_diff2(p)
    for k in (0, 1, -2, -1):
        assert np.array_equal(bits(r["path"][k]), bits(p[k]))


def test_wall_with_and_without_the_obstacle_term():
    p, occ = wall_polyline(), wall_map()
    r, d2 = run(p, occ, w_obs=0.5)
    assert r["blend"] == 1.0
    c_in = sr.clearance64(r["x0"], d2, RES, 2.0).min()
    c_out = sr.clearance64(r["path"][:, :2], d2, RES, 2.0).min()  # this frame: grid == world
    assert c_out >= c_in, (c_in, c_out)
    # smoothness alone pulls the swing back onto its chord, through the wall: lambda = 1 is refused
    r0, _ = run(p, occ, w_obs=0.0, w_fid=0.0)
    assert r0["blend"] < 1.0
    if r0["blend"] == 0:
        assert np.array_equal(bits(r0["path"]), bits(p))


def test_short_and_long_paths_are_copied_through():
    p = collinear(4)
    r, _ = run(p, empty_map())
    assert r["blend"] == 0 and r["status"] == 0 and np.array_equal(bits(r["path"]), bits(p))


def test_edt_restatement_equals_two_loops():
    rng = np.random.default_rng(5)
    for density in (0.0, 0.01, 0.1, 0.5, 1.0):
        occ = np.where(rng.random((16, 16)) < density, OCC, FREE).astype(np.float32)
        assert np.array_equal(sr.edt_brute(occ, THR), sr.edt_two_loops(occ, THR)), density
    one = np.full((16, 16), FREE, np.float32)
    one[15, 0] = THR  # occupied means >= thr
    assert np.array_equal(sr.edt_brute(one, THR), sr.edt_two_loops(one, THR))
    assert (sr.edt_brute(np.full((16, 16), FREE, np.float32), THR) == sr.CLEAR_NONE).all()


def test_cxx_smooth_path_member_compiles_and_links(tmp_path):
    """HybridAStar<float>::smooth_path (tests/cxx/smooth_main.cpp) builds with plain g++ against
    the drop-in header and links libhastar_amd.so."""
    import subprocess
    from pathlib import Path
    root = Path(__file__).resolve().parents[1]
    lib = root / "path_planning_pkg_amd" / "lib"
    assert (lib / "libhastar_amd.so").exists(), "build first (__graft_entry__.build())"
    exe = tmp_path / "smooth_main"
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", f"-I{root / 'include' / 'path_planning_pkg'}",
                    str(root / "tests" / "cxx" / "smooth_main.cpp"), f"-L{lib}", "-lhastar_amd",
                    f"-Wl,-rpath,{lib}", "-o", str(exe)], check=True, capture_output=True, text=True)
    assert exe.exists()
