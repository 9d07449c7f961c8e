"""The clearance field and the smoother (csrc/hastar_smooth.hip, the batching code at the end of
hastar_capi.cpp) where tests/test_gpu_smooth.py does not reach:

  * the field above 256 cells (runs of several cells per thread in k_edt_rows, several column
    blocks in k_edt_cols) against tests/smoother_ref.py:edt_separable and against closed forms
    at 2047 cells, and the chunk loop of hastar_clearance_field_batch;
  * the smoother at a 0.3 m resolution in a frame turned by 0.65 rad, with even and odd
    iteration counts, on a field with a row stride above 256;
  * the grid border, the options, cusps at the ends and merged cusps, all-reverse directions;
  * batch seams: empty and one-pose paths, an all-empty call, planners in the order A, B, A, B
    with one map in flight, a map changed between two calls;
  * non-finite poses.

The bar is the one of test_gpu_smooth.py: the field to equality; positions, curvatures, blend
and status to the bit; headings within 1e-5 rad.
"""
import math
import time

import numpy as np
import pytest

from tests import smoother_ref as sr
from tests import test_smoother_ref as crafted
from tests.test_gpu_smooth import assert_same, bits, device_fields, restate, set_map

pytestmark = pytest.mark.gpu

N_BIG = 2047  # 8 cells per thread in k_edt_rows, 8 column blocks in k_edt_cols
POOL_BYTES = 1 << 30  # kSmoothPoolBytes of hastar_capi.cpp


@pytest.fixture(scope="module")
def gpu():
    from path_planning_pkg_amd import planner
    planner.load_library()
    return planner


def field_planner(gpu, N):
    from path_planning_pkg_amd.capi import PlannerConfig
    return gpu.HybridAStar(PlannerConfig(grid_size=N, num_angle_bins=36))


def same(a, b):
    return (np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(bits(a[1]), bits(b[1]))
            and a[2] == b[2] and a[3] == b[3])


def batch(gpu, planners, paths, dirs=None, **opts):
    curvs = [np.zeros(len(p), np.float32) for p in paths]
    P, K, b, st = gpu.smooth_paths_batch(planners, paths, curvs, dirs, **opts)
    return [(P[k], K[k], float(b[k]), int(st[k])) for k in range(len(paths))]


def single(g, path, dirs=None, **opts):
    return g.smooth_path(path, np.zeros(len(path), np.float32), dirs, **opts)


# ------------------------------------------------------- B. the field above 256 cells ----
@pytest.mark.parametrize("N", [257, 511, 513, 1023])
def test_clearance_field_above_256_cells(gpu, N):
    """C = 2 with one thread holding a single cell and 127 idle; C = 2 with a short last run;
    C = 3 with idle threads behind the last run; C = 4 with four column blocks."""
    occ = crafted.row_pass_map(N)
    f = crafted.assert_row_pass_features(occ)
    assert f["C"] == -(-N // 256) >= 2
    g = field_planner(gpu, N)
    set_map(g, occ)
    thr = g.frame()[7]
    assert thr == crafted.THR and np.array_equal(g.get_obstacles(), occ)
    t0 = time.perf_counter()
    ref = sr.edt_separable(occ, thr)
    print(f"N = {N}: edt_separable took {time.perf_counter() - t0:.2f} s")
    dev = device_fields(gpu, [g])[0].astype(np.int64)
    wrong = dev != ref
    assert not wrong.any(), f"N = {N}: {wrong.sum()} cells differ, first at {np.argwhere(wrong)[:4].tolist()}"


@pytest.fixture(scope="module")
def big(gpu):
    t0 = time.perf_counter()
    a = field_planner(gpu, N_BIG)
    dt = time.perf_counter() - t0
    print(f"creating one {N_BIG} x {N_BIG} x 36 planner took {dt:.3f} s")
    return a, field_planner(gpu, N_BIG)


def closed_form_maps(N):
    """(tag, occupied cells or a full line, the field by its closed form in int64)."""
    i, j = np.mgrid[0:N, 0:N].astype(np.int64)

    def cells(cs):
        return np.min([(i - a) ** 2 + (j - b) ** 2 for a, b in cs], axis=0)

    L, c = N - 1, N // 2
    out = [(f"corner {k}", [k], cells([k])) for k in ((0, 0), (0, L), (L, 0), (L, L))]
    out.append(("centre", [(c, c)], cells([(c, c)])))
    out.append(("two corners", [(0, 0), (L, L)], cells([(0, 0), (L, L)])))
    out.append(("column", (slice(None), 700), (j - 700) ** 2))
    out.append(("row", (1300, slice(None)), (i - 1300) ** 2))
    return out


def big_map(where):
    m = np.full((N_BIG, N_BIG), crafted.FREE, np.float32)
    if isinstance(where, list):
        for a, b in where:
            m[a, b] = crafted.OCC
    else:
        m[where] = crafted.OCC
    return m


def test_clearance_field_closed_forms_at_2047_cells(gpu, big):
    g = big[0]
    top = 0
    for tag, where, want in closed_form_maps(N_BIG):
        set_map(g, big_map(where))
        dev = device_fields(gpu, [g])[0]
        assert dev.dtype == np.int32 and np.array_equal(dev.astype(np.int64), want), tag
        top = max(top, int(want.max()))
    assert top == 2 * (N_BIG - 1) ** 2  # the largest value a field of this size can hold


# ------------------------------------------------ C. the chunk loop of the field batch ----
def test_clearance_field_batch_runs_its_chunk_loop(gpu, big):
    import torch
    a, b = big
    forms = {tag: (where, want) for tag, where, want in closed_form_maps(N_BIG)}
    set_map(a, big_map(forms["two corners"][0]))
    set_map(b, big_map(forms["centre"][0]))
    pool = POOL_BYTES // (16 * N_BIG * N_BIG)
    n = pool + 1
    assert pool >= 1 and n > pool and n == 17  # more maps than fit: the loop runs twice
    own = []
    for g, tag in ((a, "two corners"), (b, "centre")):
        t = torch.full((1, N_BIG, N_BIG), -7, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        gpu.clearance_field_batch([g], t.data_ptr())
        assert torch.equal(t[0].cpu(), torch.from_numpy(forms[tag][1].astype(np.int32))), tag
        own.append(t[0])
    assert not torch.equal(own[0], own[1])
    dst = torch.full((n, N_BIG, N_BIG), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()  # the library writes on its own stream
    gpu.clearance_field_batch([(a, b)[k % 2] for k in range(n)], dst.data_ptr())
    for k in range(n):
        assert torch.equal(dst[k], own[k % 2]), f"slot {k}"


# ----------------------------------------------- D. the smoother off the exact grid ----
def planner3(gpu, N, frame):
    from path_planning_pkg_amd.capi import PlannerConfig
    g = gpu.HybridAStar(PlannerConfig(grid_size=N, grid_resolution=crafted.RES3, num_angle_bins=36))
    g.update_goal(crafted.GOAL3, crafted.START3)
    got = g.frame()
    assert np.array_equal(bits(got), bits(frame)), (got.tolist(), frame.tolist())
    assert abs(math.atan2(-float(got[1]), float(got[0])) - 0.65) < 1e-3  # the grid heading
    return g


@pytest.fixture(scope="module")
def g100(gpu):
    return planner3(gpu, 100, crafted.FRAME3)


@pytest.fixture(scope="module")
def g513(gpu):
    return planner3(gpu, 513, crafted.FRAME513)


def valid_on_map(path, frame, occ):
    """Judged in float64 as tests/test_gpu_relaxed.py:check_valid does: every pose inside the
    grid and on a free floor or round cell."""
    N, res, thr = len(occ), float(frame[6]), frame[7]
    gxy = crafted.to_grid(frame, path)
    ci, cj = np.floor(gxy[:, 0] / res + 1e-6).astype(int), np.floor(gxy[:, 1] / res + 1e-6).astype(int)
    ri, rj = np.rint(gxy[:, 0] / res).astype(int), np.rint(gxy[:, 1] / res).astype(int)
    if not ((ci >= 0) & (ci < N) & (cj >= 0) & (cj < N)).all():
        return False
    rin = (ri >= 0) & (ri < N) & (rj >= 0) & (rj < N)
    free_r = np.zeros(len(ci), bool)
    free_r[rin] = occ[ri[rin], rj[rin]] < thr
    return bool(((occ[ci, cj] < thr) | free_r).all())


def gaps64(path):
    p = np.asarray(path, np.float64)
    return float(np.hypot(np.diff(p[:, 0]), np.diff(p[:, 1])).max())


def check_off_grid(gpu, g, frame, N, off):
    occ = crafted.blocks_map3(N, *off)
    set_map(g, occ)
    d2 = sr.edt_separable(occ, crafted.THR)
    assert np.array_equal(device_fields(gpu, [g])[0], d2)
    res = float(frame[6])
    blends = []
    for n in crafted.WAVY_LENGTHS:
        p = crafted.wavy3(frame, n, *off)
        z = np.zeros(n, np.float32)
        for it in crafted.WAVY_ITERATIONS:
            what = f"N = {N}, n = {n}, {it} iterations"
            dev = g.smooth_path(p, z, iterations=it)
            ref, _ = restate(g, p, z, None, d2, iterations=it)
            print(f"{what}: blend {dev[2]}")
            assert_same(dev, ref, what)
            blends.append(dev[2])
            # the promises, in float64
            assert dev[2] > 0, what
            for k in (0, 1, -2, -1):
                assert np.array_equal(bits(dev[0][k]), bits(p[k])), f"{what}: end point {k} moved"
            assert valid_on_map(dev[0], frame, occ), what
            assert gaps64(dev[0]) <= 1.25 * gaps64(p) + 1e-3, what
            j_in = sr.objective(ref["x0"], ref["x0"], d2, res)
            j_out = sr.objective(ref["xs"], ref["x0"], d2, res)
            assert j_out <= j_in, f"{what}: J {j_in} -> {j_out}"
    assert 1.0 in blends and min(blends) < 1.0, blends


def test_smoother_off_the_exact_grid(gpu, g100):
    check_off_grid(gpu, g100, crafted.FRAME3, 100, (0, 0))


def test_smoother_reads_a_field_wider_than_256_cells(gpu, g513):
    check_off_grid(gpu, g513, crafted.FRAME513, 513, crafted.OFF513)


# ------------------------------------------------------ E. border, options, cusps ----
def test_border_of_the_grid(gpu, g100):
    occ = crafted.far_cell_map()
    set_map(g100, occ)
    d2 = sr.edt_brute(occ, crafted.THR)
    assert np.array_equal(device_fields(gpu, [g100])[0], d2)
    for axis, cells, accepted in crafted.BORDER_CASES:
        p = crafted.border_path(crafted.FRAME3, axis, cells)
        z = np.zeros(len(p), np.float32)
        dev = g100.smooth_path(p, z)
        ref, _ = restate(g100, p, z, None, d2)
        assert_same(dev, ref, f"border: axis {axis}, {cells:+} cells")
        assert dev[2] == float(ref["blend"])
        if accepted is not None:
            assert (dev[2] > 0) == accepted, (axis, cells, dev[2])


def test_options(gpu, g100):
    occ = crafted.blocks_map3()
    set_map(g100, occ)
    d2 = sr.edt_brute(occ, crafted.THR)
    p = crafted.wavy3(crafted.FRAME3, 65)
    z = np.zeros(len(p), np.float32)
    base = g100.smooth_path(p, z)
    assert_same(base, restate(g100, p, z, None, d2)[0], "default options")
    differ = 0
    for opts in crafted.option_cases(p):
        dev = g100.smooth_path(p, z, **opts)
        ropts = dict(opts)
        kmax = ropts.pop("kappa_max", float(g100.motion_tables()["curv_abs"].max()))
        ref = sr.smooth_ref(p, z, None, g100.frame(), occ, d2, kmax, **ropts)
        assert_same(dev, ref, f"options {opts}")
        differ += not same(dev, base)
    assert differ >= 3, differ


def test_directions_and_cusps(gpu, g100):
    occ = crafted.far_cell_map()
    set_map(g100, occ)
    d2 = sr.edt_brute(occ, crafted.THR)
    for tag, n, d, fixed in crafted.cusp_cases():
        p = crafted.zigzag3(n=n)
        z = np.zeros(n, np.float32)
        dev = g100.smooth_path(p, z, d)
        ref, _ = restate(g100, p, z, d, d2)
        assert_same(dev, ref, tag)
        assert dev[2] > 0, tag
        assert np.array_equal(bits(dev[0][fixed]), bits(p[fixed])), f"{tag}: a fixed pose moved"
        free = np.setdiff1d(np.arange(n), fixed)
        assert (bits(dev[0][free, :2]) != bits(p[free, :2])).any(axis=1).all(), f"{tag}: a free pose stayed"
    p = crafted.zigzag3()
    z = np.zeros(len(p), np.float32)
    fwd, rev = g100.smooth_path(p, z), g100.smooth_path(p, z, -np.ones(len(p), np.int8))
    assert np.array_equal(bits(rev[0][:, :2]), bits(fwd[0][:, :2])) and np.array_equal(bits(rev[1]), bits(fwd[1]))
    turn = np.abs(rev[0][2:-2, 2].astype(np.float64) - fwd[0][2:-2, 2].astype(np.float64))
    assert np.allclose(turn, math.pi, atol=1e-6), turn


# ------------------------------------------------------------------ F. batch seams ----
def test_batch_of_mixed_lengths_and_empty_paths(gpu, g100):
    set_map(g100, crafted.blocks_map3())
    lens = (0, 65, 1, 0, 4, 257, 0)
    paths = [crafted.wavy3(crafted.FRAME3, max(n, 2))[:n] for n in lens]
    got = batch(gpu, [g100] * len(lens), paths)
    for k, n in enumerate(lens):
        assert got[k][0].shape == (n, 3) and got[k][1].shape == (n,), n
        if n == 0:
            assert got[k][2] == 0 and got[k][3] == 0
            continue
        assert same(got[k], single(g100, paths[k])), f"path {k} of {n} poses differs from its single call"
        if n < 5:
            assert got[k][2] == 0 and got[k][3] == 0 and np.array_equal(bits(got[k][0]), bits(paths[k]))
    assert got[1][2] > 0 and got[5][2] > 0, [r[2] for r in got]
    # a call whose paths are all empty is no error
    for r in batch(gpu, [g100] * 3, [np.zeros((0, 3), np.float32)] * 3):
        assert r[0].shape == (0, 3) and r[1].shape == (0,) and r[2] == 0 and r[3] == 0
    r = single(g100, np.zeros((0, 3), np.float32))
    assert r[0].shape == (0, 3) and r[2] == 0 and r[3] == 0


def test_planners_alternate_with_one_map_in_flight(gpu, g100):
    other = planner3(gpu, 100, crafted.FRAME3)
    ma, mb = crafted.moved_block_maps()
    set_map(g100, ma)
    set_map(other, mb)
    planners = [g100, other, g100, other]
    paths = [crafted.wavy3(crafted.FRAME3, n, amp=0.3) for n in (65, 66, 120, 121)]
    chunked = batch(gpu, planners, paths, max_maps_in_flight=1)
    plain = batch(gpu, planners, paths)
    for k in range(4):
        assert chunked[k][2] > 0
        assert same(chunked[k], single(planners[k], paths[k])), f"path {k}: chunked batch differs from its single call"
        assert same(chunked[k], plain[k]), f"path {k}: chunked batch differs from the plain batch"
    # the two maps do tell: the same path on the other planner comes out differently
    assert not same(single(g100, paths[0]), single(other, paths[0]))


def test_map_changed_between_two_calls(gpu, g100):
    ma, mb = crafted.moved_block_maps()
    p = crafted.wavy3(crafted.FRAME3, 65, amp=0.3)
    z = np.zeros(len(p), np.float32)
    set_map(g100, ma)
    first = g100.smooth_path(p, z)
    ref_a, _ = restate(g100, p, z)
    set_map(g100, mb)
    ref_b, _ = restate(g100, p, z)
    assert not np.array_equal(bits(ref_a["path"]), bits(ref_b["path"]))  # the case discriminates
    second = g100.smooth_path(p, z)
    assert_same(first, ref_a, "before the map changed")
    assert_same(second, ref_b, "after the map changed")
    assert not same(first, second)


# ------------------------------------------------------------ G. non-finite poses ----
@pytest.mark.parametrize("index, coord, value", [(11, 0, math.nan), (1, 1, math.nan), (11, 1, math.inf), (12, 0, -math.inf)])
def test_non_finite_pose_is_refused_and_leaves_its_neighbour_alone(gpu, g100, index, coord, value):
    set_map(g100, crafted.far_cell_map())
    bad = crafted.collinear3()
    assert len(bad) == 24 and bool(sr.fixed_mask(24)[index]) == (index == 1)
    bad[index, coord] = value
    healthy = crafted.zigzag3()
    alone = single(g100, healthy)
    assert alone[2] > 0
    for order in ((0, 1), (1, 0)):
        paths = [(bad, healthy)[k] for k in order]
        got = batch(gpu, [g100, g100], paths)
        b, h = got[order.index(0)], got[order.index(1)]
        assert b[2] == 0 and b[3] == 0
        assert np.array_equal(bits(b[0]), bits(bad)) and np.array_equal(bits(b[1]), bits(np.zeros(24)))
        assert same(h, alone)
