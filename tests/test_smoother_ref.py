"""The numpy restatement of the clearance field and the smoother (tests/smoother_ref.py) on its
own, without a GPU: the properties the smoother promises, shown on the arithmetic that
tests/test_gpu_smooth.py then holds the device to, bit for bit.

The crafted cases live in a 64 x 64 map at 0.5 m whose grid frame equals the world frame
(goal (25.5, 16, 0) seen from a start on the same y: heading 0, goal cell (51, 32)).  The cases
of tests/test_gpu_smooth_edges.py live at 0.3 m in a frame turned by 0.65 rad (FRAME3, FRAME513);
their builders are here so that the CPU tests can show, on the restatement alone, that each case
does what it is there for.
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


def test_edt_separable_equals_two_loops_and_brute_force():
    """The large-map reference (row distances, then a plain minimum over the rows) against the
    definition on small maps and against the brute force at 257 cells."""
    rng = np.random.default_rng(5)
    for density in (0.0, 0.01, 0.1, 0.5, 1.0):  # the maps of test_edt_restatement_equals_two_loops
        occ = np.where(rng.random((16, 16)) < density, OCC, FREE).astype(np.float32)
        assert np.array_equal(sr.edt_separable(occ, THR), sr.edt_two_loops(occ, THR)), density
    one = np.full((16, 16), FREE, np.float32)
    one[15, 0] = THR
    assert np.array_equal(sr.edt_separable(one, THR), sr.edt_two_loops(one, THR))
    assert (sr.edt_separable(np.full((16, 16), FREE, np.float32), THR) == sr.CLEAR_NONE).all()
    occ = row_pass_map(40)  # empty rows, rows with only their end cells, a full row
    assert np.array_equal(sr.edt_separable(occ, THR), sr.edt_two_loops(occ, THR))
    sparse = np.where(np.random.default_rng(257).random((257, 257)) < 0.003, OCC, FREE).astype(np.float32)
    assert 100 < (sparse >= THR).sum() < 400
    assert np.array_equal(sr.edt_separable(sparse, THR), sr.edt_brute(sparse, THR))


# ------------------------------------------- maps that exercise the field's row pass ----
def row_pass_map(N, seed=0):
    """A map for k_edt_rows at N > 256 (tests/test_gpu_smooth_edges.py): the density of row i
    rises from 0 to about 0.5; nine rows are empty (row 0, six adjacent rows and two single
    ones), three rows hold only cell 0, only cell N - 1, or only both, and one row is full."""
    rng = np.random.default_rng(1000 * seed + N)
    p = 0.5 * np.arange(N) / (N - 1)
    m = np.where(rng.random((N, N)) < p[:, None], OCC, FREE).astype(np.float32)
    s = row_pass_rows(N)
    m[s["empty"]] = FREE
    for k, cells in (("first", [0]), ("last", [N - 1]), ("both", [0, N - 1])):
        m[s[k]] = FREE
        m[s[k], cells] = OCC
    m[s["full"]] = THR  # occupied means >= thr
    return m


def row_pass_rows(N):
    a, b = N // 3, (2 * N) // 3
    return dict(empty=[0] + list(range(a, a + 6)) + [N // 2 + 3, N - 5], first=b, last=b + 2, both=b + 4, full=N - 2)


def row_pass_features(m, threads=256):
    """What row_pass_map promises, read back from the map itself (asserted by the CPU test at
    every size the GPU test uses, and again by the GPU test before the device is asked)."""
    N = len(m)
    o = m >= THR
    cnt = o.sum(axis=1)
    empty = np.nonzero(cnt == 0)[0]
    C = -(-N // threads)
    pad = np.zeros((N, threads * C), bool)
    pad[:, :N] = o
    runs = pad.reshape(N, threads, C).sum(axis=2)  # occupied cells of thread t's run, per row
    used = -(-N // C)  # threads whose run begins inside the row
    gap = (runs[:, 1:used - 1] == 0) & (runs[:, :used - 2] > 0) & (runs[:, 2:used] > 0)
    q = N // 4
    return dict(
        C=C, empty_rows=len(empty), row0_empty=bool(cnt[0] == 0), adjacent_empty=bool((np.diff(empty) == 1).any()),
        only_first=bool(((cnt == 1) & o[:, 0]).any()), only_last=bool(((cnt == 1) & o[:, -1]).any()),
        only_both=bool(((cnt == 2) & o[:, 0] & o[:, -1]).any()), full_rows=int((cnt == N).sum()),
        density_low=float(o[:q].mean()), density_high=float(o[-q:].mean()),
        run_with_two=bool((runs >= 2).any()), empty_run_between=bool(gap.any()))


def assert_row_pass_features(m):
    f = row_pass_features(m)
    assert f["empty_rows"] >= 8 and f["row0_empty"] and f["adjacent_empty"], f
    assert f["only_first"] and f["only_last"] and f["only_both"] and f["full_rows"] == 1, f
    assert f["density_low"] < 0.1 and f["density_high"] > 0.35, f
    assert f["run_with_two"] and f["empty_run_between"], f
    return f


def test_row_pass_maps_have_their_features():
    for N, C in ((257, 2), (511, 2), (513, 3), (1023, 4)):
        assert assert_row_pass_features(row_pass_map(N))["C"] == C


# ----------------------------------------------------- a frame off the exact grid ----
# 0.3 m cells and a grid heading near 0.65 rad, the goal away from the world's origin: x / res is
# a real division and both rotations are real products.
RES3 = 0.3
GOAL3 = [7.0, -3.0, 0.0]
START3 = [float(np.float32(7.0 - 12.0 * math.cos(0.65))), float(np.float32(-3.0 - 12.0 * math.sin(0.65))), 0.0]


def hand_frame(N, res=RES3, goal=GOAL3, start=START3):
    """hastar_update_goal's frame by hand: the grid heading is atan2f of the float32 differences,
    rot = cosf / sinf of minus the heading (taken in float64 and rounded once, which a correctly
    rounded float32 function equals), the goal sits in cell (round(0.8 N), round(N / 2))."""
    f = np.float32
    g, s, res = np.asarray(goal, f), np.asarray(start, f), f(res)
    h = f(math.atan2(float(g[1] - s[1]), float(g[0] - s[0])))
    ci, cj = math.floor(0.8 * N + 0.5), math.floor(0.5 * N + 0.5)  # std::round
    return np.array([f(math.cos(float(-h))), f(math.sin(float(-h))), g[0], g[1], f(ci) * res, f(cj) * res, res, THR], f)


FRAME3 = hand_frame(100)
FRAME513 = hand_frame(513)


def to_world(frame, gxy):
    """Grid-frame points to the world frame, in float64 (the smoother's store expression)."""
    rc, rs, wgx, wgy, gx0, gy0 = (float(v) for v in frame[:6])
    a = np.asarray(gxy, np.float64) - [gx0, gy0]
    return np.column_stack([a[:, 0] * rc + a[:, 1] * rs + wgx, -a[:, 0] * rs + a[:, 1] * rc + wgy])


def to_grid(frame, xy):
    """World-frame points to the grid frame, in float64."""
    rc, rs, wgx, wgy, gx0, gy0 = (float(v) for v in frame[:6])
    d = np.asarray(xy, np.float64)[:, :2] - [wgx, wgy]
    return np.column_stack([d[:, 0] * rc - d[:, 1] * rs + gx0, d[:, 0] * rs + d[:, 1] * rc + gy0])


def blocks_map3(N=100, oi=0, oj=0):
    """Two blocks, 6 x 5 cells of 0.3 m, shifted by (oi, oj) cells."""
    m = np.full((N, N), FREE, np.float32)
    m[oi + 25:oi + 31, oj + 59:oj + 64] = OCC  # x 7.5 .. 9.0 m, y 17.7 .. 18.9 m
    m[oi + 67:oi + 73, oj + 37:oj + 42] = OCC  # x 20.1 .. 21.6 m, y 11.1 .. 12.3 m
    return m


def wavy3(frame, n, oi=0, oj=0, amp=1.5):
    """n poses along a sine between the blocks of blocks_map3 (1.2 m from each at its crests, so
    within d_max of both), with a 1 mm ripple: built in the grid frame, returned in the world's."""
    k = np.arange(n - 1, -1, -1, dtype=np.float64) / max(n - 1, 1)
    rng = np.random.default_rng(n)
    res = float(frame[6])
    x = 2.0 + 25.0 * k + oi * res
    y = 15.0 + amp * np.sin(2 * math.pi * k) + 1e-3 * rng.standard_normal(n) + oj * res
    return with_headings(to_world(frame, np.column_stack([x, y])))


OFF513 = (300, 200)  # the 513-cell cases sit at field rows above 256
WAVY_LENGTHS = (65, 300)
WAVY_ITERATIONS = (200, 201, 3, 1)


def run3(path, occ, frame=FRAME3, dirs=None, d2=None, **opts):
    if d2 is None:
        d2 = sr.edt_brute(occ, THR)
    return sr.smooth_ref(path, np.zeros(len(path), np.float32), dirs, frame, occ, d2, KAPPA, **opts), d2


def moved(r, path):
    return (bits(r["path"][:, :2]) != bits(path[:, :2])).any(axis=1)


def test_off_grid_cases_are_not_vacuous():
    """Every sine case of tests/test_gpu_smooth_edges.py is accepted at some lambda and moves more
    than half of its poses, in both planners' frames; an odd iteration count gives other bits than
    the even one next to it."""
    for frame, N, (oi, oj) in ((FRAME3, 100, (0, 0)), (FRAME513, 513, OFF513)):
        occ = blocks_map3(N, oi, oj)
        d2 = sr.edt_separable(occ, THR)
        for n in WAVY_LENGTHS:
            p = wavy3(frame, n, oi, oj)
            res = {}
            for it in WAVY_ITERATIONS:
                res[it], _ = run3(p, occ, frame, d2=d2, iterations=it)
                print(f"N = {N}, n = {n}, {it} iterations: blend {res[it]['blend']}, {moved(res[it], p).sum()} poses moved")
                assert res[it]["blend"] > 0 and res[it]["status"] == 0
                assert moved(res[it], p).sum() > n // 2
            assert not np.array_equal(bits(res[200]["xs"]), bits(res[201]["xs"]))
            assert not np.array_equal(bits(res[200]["path"]), bits(res[201]["path"]))
        # the obstacle term is at work: the sine comes within d_max of both blocks
        c = sr.clearance64(to_grid(frame, wavy3(frame, 65, oi, oj)), d2, RES3, 2.0)
        assert c.min() < 1.5


# ------------------------------------------------------------ border of the grid ----
def far_cell_map(N=100):
    m = np.full((N, N), FREE, np.float32)
    m[5, 5] = OCC
    return m


def border_path(frame, axis, cells, n=40, N=100):
    """n poses along the last grid row (axis 0: x = (N - 1 + cells) res) or along column 0 (axis 1:
    y = cells * res), 0.3 m apart, with a 0.02 m zig-zag across the line."""
    res = float(frame[6])
    k = np.arange(n - 1, -1, -1, dtype=np.float64)
    along = (20.0 + k) * res
    across = ((N - 1 + cells) if axis == 0 else cells) * res + 0.02 * ((k.astype(int) % 2) * 2 - 1)
    g = np.column_stack([across, along] if axis == 0 else [along, across])
    return with_headings(to_world(frame, g))


# (axis, offset in cells from the centre of row N - 1 / column 0, accepted?).  The centre of cell
# i is at i * res; a point is refused once its floor or its round cell leaves [0, N - 1].  Past
# row N - 1 that happens at +0.5 cells (the round cell becomes N).  Before column 0 it happens
# at the centre itself (the floor cell becomes -1), so both -0.2 and -0.6 are refused there and
# the accepted side of that edge is +0.2.
BORDER_CASES = ((0, 0.2, True), (0, 0.45, None), (0, 0.6, False), (1, -0.2, False), (1, -0.6, False), (1, 0.2, True))


def test_border_paths_fall_on_both_sides_of_the_accept_rule():
    occ = far_cell_map()
    d2 = sr.edt_brute(occ, THR)
    for axis, cells, accepted in BORDER_CASES:
        p = border_path(FRAME3, axis, cells)
        r, _ = run3(p, occ, d2=d2)
        print(f"axis {axis}, {cells:+} cells: blend {r['blend']}")
        if accepted is None:
            continue
        assert (r["blend"] > 0) == accepted, (axis, cells, r["blend"])
        if accepted:
            assert moved(r, p).sum() > len(p) // 2
        else:
            assert np.array_equal(bits(r["path"]), bits(p))
            assert not np.array_equal(bits(r["xs"]), bits(r["x0"]))  # it was smoothed, then refused


# ------------------------------------------------------------ options and cusps ----
def largest_curvature(path):
    """The largest Menger curvature over the interior poses, in float64."""
    p = np.asarray(path, np.float64)[:, :2]
    a, b, c = p[:-2], p[1:-1], p[2:]
    cr = np.abs((b - a)[:, 0] * (c - b)[:, 1] - (b - a)[:, 1] * (c - b)[:, 0])
    den = np.hypot(*(b - a).T) * np.hypot(*(c - b).T) * np.hypot(*(c - a).T)
    return float((2 * cr / den).max())


def option_cases(path):
    k = largest_curvature(path)
    return (dict(kappa_max=0.5 * k), dict(kappa_max=100.0 * k), dict(d_max=0.75), dict(d_max=6.0), dict(w_smooth=0))


def run3k(path, occ, d2, **opts):
    """run3 with kappa_max as the library takes it: an option that replaces the vehicle's."""
    kmax = opts.pop("kappa_max", KAPPA)
    return sr.smooth_ref(path, np.zeros(len(path), np.float32), None, FRAME3, occ, d2, kmax, **opts)


def test_options_change_the_result():
    occ = blocks_map3()
    d2 = sr.edt_brute(occ, THR)
    p = wavy3(FRAME3, 65)
    base = run3k(p, occ, d2)
    differ = 0
    for opts in option_cases(p):
        r = run3k(p, occ, d2, **opts)
        d = r["blend"] != base["blend"] or not np.array_equal(bits(r["path"]), bits(base["path"]))
        print(f"{opts}: blend {r['blend']} (default {base['blend']}), differs {d}")
        differ += d
    assert differ >= 3, differ


def zigzag3(frame=FRAME3, n=30):
    k = np.arange(n - 1, -1, -1, dtype=np.float64)
    return with_headings(to_world(frame, np.column_stack([4.0 + 0.5 * k, 12.0 + 0.2 * ((k.astype(int) % 2) * 2 - 1)])))


def collinear3(frame=FRAME3, n=24):
    k = np.arange(n - 1, -1, -1, dtype=np.float64)
    return with_headings(to_world(frame, np.column_stack([4.0 + 0.5 * k, 8.0 + 0.25 * k])))


def cusp_cases(n=30):
    """(tag, n, dir, the poses that must keep their input bits)."""
    def dirs(n, flips):
        d, s = np.ones(n, np.int8), 1
        for i in range(n):
            d[i] = s
            if i in flips:
                s = -s
        return d
    return (("all reverse", n, -np.ones(n, np.int8), [0, 1, n - 2, n - 1]),
            ("cusp at 0", n, dirs(n, [0]), [0, 1, n - 2, n - 1]),
            ("cusp at n - 2", n, dirs(n, [n - 2]), [0, 1, n - 3, n - 2, n - 1]),
            ("cusps at 10 and 12", n, dirs(n, [10, 12]), [0, 1, 9, 10, 11, 12, 13, n - 2, n - 1]),
            ("5 poses, cusp at 1", 5, dirs(5, [1]), [0, 1, 2, 3, 4]))


def test_cusps_fix_their_neighbourhoods():
    occ = far_cell_map()
    d2 = sr.edt_brute(occ, THR)
    for tag, n, d, fixed in cusp_cases():
        p = zigzag3(n=n)
        assert np.array_equal(np.nonzero(sr.fixed_mask(n, d))[0], fixed), tag
        r, _ = run3(p, occ, dirs=d, d2=d2)
        assert r["blend"] > 0, tag
        mv = moved(r, p)
        assert not mv[fixed].any() and mv.sum() == n - len(fixed), tag
        assert np.array_equal(bits(r["path"][fixed]), bits(p[fixed])), tag
    # dir = -1 everywhere: the positions of the forward run, every moved heading turned by pi
    p = zigzag3()
    fwd, _ = run3(p, occ, d2=d2)
    rev, _ = run3(p, occ, dirs=-np.ones(30, np.int8), d2=d2)
    assert np.array_equal(bits(rev["path"][:, :2]), bits(fwd["path"][:, :2]))
    turn = np.abs(rev["path"][2:-2, 2].astype(np.float64) - fwd["path"][2:-2, 2].astype(np.float64))
    assert np.allclose(turn, math.pi, atol=1e-6)


def test_a_moved_block_changes_the_result():
    """The two maps of the GPU test that swaps a planner's map between two calls."""
    p = wavy3(FRAME3, 65, amp=0.3)
    a, b = moved_block_maps()
    ra, _ = run3(p, a)
    rb, _ = run3(p, b)
    assert ra["blend"] > 0 and rb["blend"] > 0
    assert not np.array_equal(bits(ra["path"]), bits(rb["path"]))


def moved_block_maps():
    """One block above the middle of the nearly straight wavy3(.., amp=0.3), or below it."""
    a, b = (np.full((100, 100), FREE, np.float32) for _ in range(2))
    a[45:51, 53:57] = OCC  # y 15.9 .. 16.8 m, over the path (y about 15 m)
    b[45:51, 44:48] = OCC  # y 13.2 .. 14.1 m, under it
    return a, b


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
