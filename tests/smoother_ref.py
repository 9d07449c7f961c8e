"""numpy restatement of the clearance field and the path smoother (csrc/hastar_smooth.hip,
DESIGN.md §4.7).  Not an oracle of the reference (which has no smoother): it restates the
library's documented arithmetic so that the device result can be compared to the bit.

  * edt_brute: the squared Euclidean distance transform by brute force in int64 (min over the
    occupied cells, by broadcasting); edt_two_loops: the same with plain Python loops;
    edt_separable: the same for maps too large for either (row distances, then a plain minimum
    over the rows).
  * smooth_ref: the smoother, the blend and the accept rule in float32, one operation at a
    time in the kernel's order.  It takes the frame from hastar_debug_frame and the map from
    get_obstacles().
  * objective / sum_second_diff2: float64 figures for the property checks.
"""
import numpy as np

f32 = np.float32
CLEAR_NONE = 0x7fffffff
MAX_POINTS = 8192
ENOSPC = -28
PI_F = f32(np.pi)


def edt_brute(occ, thr):
    """d2[i, j] = min over occupied (i', j') of (i - i')^2 + (j - j')^2; occupied = occ >= thr."""
    occ = np.asarray(occ, np.float32)
    N = occ.shape[0]
    ii, jj = np.nonzero(occ >= f32(thr))
    out = np.full((N, N), CLEAR_NONE, np.int64)
    if len(ii) == 0:
        return out
    ii, jj = ii.astype(np.int64), jj.astype(np.int64)
    j = np.arange(N, dtype=np.int64)
    dj2 = (j[:, None] - jj[None, :]) ** 2
    for i in range(N):
        out[i] = (dj2 + ((i - ii) ** 2)[None, :]).min(axis=1)
    return out


def edt_two_loops(occ, thr):
    """The definition, one cell and one obstacle at a time (small maps only)."""
    N = len(occ)
    cells = [(a, b) for a in range(N) for b in range(N) if occ[a][b] >= thr]
    out = np.full((N, N), CLEAR_NONE, np.int64)
    for i in range(N):
        for j in range(N):
            best = CLEAR_NONE
            for a, b in cells:
                d = (i - a) * (i - a) + (j - b) * (j - b)
                if d < best:
                    best = d
            out[i, j] = best
    return out


def edt_separable(occ, thr):
    """The same field for large maps, O(N^3) whatever the occupancy: per row u the exact distance
    g[u, j] along j to the row's nearest occupied cell (by broadcasting against the row's occupied
    indices), then per output row i the minimum over u of (i - u)^2 + g[u, j]^2 in int64.  Rows
    without an occupied cell carry a sentinel above every real value.  No scan, no envelope and
    no separator: a different decomposition from the kernel's two passes."""
    occ = np.asarray(occ, np.float32)
    N = occ.shape[0]
    m = occ >= f32(thr)
    out = np.full((N, N), CLEAR_NONE, np.int64)
    if not m.any():
        return out
    none = np.int64(1) << 40  # 2 (N - 1)^2 < 2^31 for every N the library takes
    j = np.arange(N, dtype=np.int64)
    g2 = np.full((N, N), none, np.int64)
    for u in range(N):
        jj = np.nonzero(m[u])[0].astype(np.int64)
        if len(jj):
            g2[u] = np.abs(j[:, None] - jj[None, :]).min(axis=1) ** 2
    for i in range(N):
        out[i] = (((i - j) ** 2)[:, None] + g2).min(axis=0)
    return out


def fixed_mask(n, dirs=None):
    """Points that never move: 0, 1, n-2, n-1 and every cusp i (dir[i] != dir[i+1]) with i-1, i+1."""
    fx = np.zeros(n, bool)
    fx[:2] = True
    fx[max(n - 2, 0):] = True
    if dirs is not None:
        d = np.asarray(dirs, np.int8)
        for i in np.nonzero(d[:-1] != d[1:])[0]:
            fx[max(i - 1, 0):i + 2] = True
    return fx


def _menger(ax, ay, bx, by, cx, cy):
    abx, aby, bcx, bcy, acx, acy = bx - ax, by - ay, cx - bx, cy - by, cx - ax, cy - ay
    cr = np.abs(abx * bcy - aby * bcx)
    l1 = np.sqrt(abx * abx + aby * aby)
    l2 = np.sqrt(bcx * bcx + bcy * bcy)
    l3 = np.sqrt(acx * acx + acy * acy)
    den = (l1 * l2) * l3
    with np.errstate(divide="ignore", invalid="ignore"):
        k = (cr + cr) / den
    return np.where(den > 0, k, f32(0)).astype(np.float32)


def _clamp_cell(f, N):
    f = np.where(~(f >= 0), f32(0), np.where(f > f32(N - 1), f32(N - 1), f))
    return f.astype(np.int64)


def _roundf(u):
    """C roundf (halves away from zero), exactly."""
    a = np.abs(u)
    r = np.floor(a)
    r = r + ((a - r) >= f32(0.5)).astype(np.float32)
    return np.copysign(r, u).astype(np.float32)


def _clear_cells(d2, i, j, res, d_max):
    v = d2[i, j]
    with np.errstate(invalid="ignore"):
        c = res * np.sqrt(np.where(v == CLEAR_NONE, 0, v).astype(np.float32))
    return np.where(v == CLEAR_NONE, d_max, c).astype(np.float32)


def _max(a):
    return f32(a.max()) if len(a) else f32(0)


def smooth_ref(path, curv, dirs, frame, occ, d2, kappa_max, w_smooth=1.0, w_obs=0.5, w_fid=0.05, d_max=2.0,
               iterations=200):
    """The library's smoother on one path.  frame = hastar_debug_frame's 8 floats; occ the
    planner's log-odds map; d2 its clearance field (edt_brute).  Weights are taken as given (0
    switches a term off).  Returns a dict: path, curvature, blend, status, and the grid-frame
    arrays x0 (input), xs (after the last iteration), fixed."""
    path = np.ascontiguousarray(path, np.float32).reshape(-1, 3)
    curv = np.ascontiguousarray(curv, np.float32)
    n = len(path)
    if n < 5 or n > MAX_POINTS:
        return dict(path=path.copy(), curvature=curv.copy(), blend=f32(0), status=ENOSPC if n > MAX_POINTS else 0)
    rc, rs, wgx, wgy, gx0, gy0, res, thr = (f32(v) for v in frame)
    occ = np.asarray(occ, np.float32)
    N = occ.shape[0]
    ws, wo, wf, d_max = f32(w_smooth), f32(w_obs), f32(w_fid), f32(d_max)
    ws2, wo2, wf2 = ws + ws, wo + wo, wf + wf
    alpha = f32(1) / ((f32(32) * ws + f32(4) * wo) + f32(2) * wf)
    # world -> grid frame
    dx, dy = path[:, 0] - wgx, path[:, 1] - wgy
    x0 = ((dx * rc - dy * rs) + gx0).astype(np.float32)
    y0 = ((dx * rs + dy * rc) + gy0).astype(np.float32)
    fx = fixed_mask(n, dirs)
    idx = np.nonzero(~fx)[0]

    def gaps(x, y):
        ex, ey = x[1:] - x[:-1], y[1:] - y[:-1]
        return _max(np.sqrt(ex * ex + ey * ey))

    def kappas(x, y):
        return _max(_menger(x[idx - 1], y[idx - 1], x[idx], y[idx], x[idx + 1], y[idx + 1]))

    gap_lim = f32(1.25) * gaps(x0, y0)
    kap_lim = max(f32(kappa_max), kappas(x0, y0))
    x, y = x0.copy(), y0.copy()
    i = idx
    for _ in range(int(iterations)):
        if len(i) == 0:
            break
        xi, yi = x[i], y[i]
        dmx = (x[i - 2] + xi) - (x[i - 1] + x[i - 1])
        d0x = (x[i - 1] + x[i + 1]) - (xi + xi)
        dpx = (xi + x[i + 2]) - (x[i + 1] + x[i + 1])
        dmy = (y[i - 2] + yi) - (y[i - 1] + y[i - 1])
        d0y = (y[i - 1] + y[i + 1]) - (yi + yi)
        dpy = (yi + y[i + 2]) - (y[i + 1] + y[i + 1])
        gsx = ws2 * ((dmx + dpx) - (d0x + d0x))
        gsy = ws2 * ((dmy + dpy) - (d0y + d0y))
        gfx = wf2 * (xi - x0[i])
        gfy = wf2 * (yi - y0[i])
        u, v = xi / res, yi / res
        fi, fj = np.floor(u), np.floor(v)
        fu, fv = u - fi, v - fj
        i0, i1 = _clamp_cell(fi, N), _clamp_cell(fi + f32(1), N)
        j0, j1 = _clamp_cell(fj, N), _clamp_cell(fj + f32(1), N)
        c00, c01 = _clear_cells(d2, i0, j0, res, d_max), _clear_cells(d2, i0, j1, res, d_max)
        c10, c11 = _clear_cells(d2, i1, j0, res, d_max), _clear_cells(d2, i1, j1, res, d_max)
        a0, a1 = c00 + fv * (c01 - c00), c10 + fv * (c11 - c10)
        b0, b1 = c00 + fu * (c10 - c00), c01 + fu * (c11 - c01)
        c = a0 + fu * (a1 - a0)
        m = np.where(c < d_max, wo2 * (d_max - c), f32(0)).astype(np.float32)
        gox, goy = m * ((a1 - a0) / res), m * ((b1 - b0) / res)
        xn, yn = x.copy(), y.copy()
        xn[i] = xi - alpha * ((gsx + gfx) - gox)
        yn[i] = yi - alpha * ((gsy + gfy) - goy)
        x, y = xn, yn
    xs, ys = x, y
    assert xs.dtype == np.float32 and ys.dtype == np.float32
    blend, bx, by = f32(0), None, None
    hi = f32(N - 1)
    for lam in (f32(1), f32(0.5), f32(0.25), f32(0.125)):
        tx, ty = x0.copy(), y0.copy()
        tx[i] = x0[i] + lam * (xs[i] - x0[i])
        ty[i] = y0[i] + lam * (ys[i] - y0[i])
        u, v = tx[i] / res, ty[i] / res
        fi, fj, ri, rj = np.floor(u), np.floor(v), _roundf(u), _roundf(v)
        ok = (fi >= 0) & (fi <= hi) & (fj >= 0) & (fj <= hi) & (ri >= 0) & (ri <= hi) & (rj >= 0) & (rj <= hi)
        w = np.nonzero(ok)[0]
        free = np.zeros(len(i), bool)
        free[w] = ~(occ[fi[w].astype(np.int64), fj[w].astype(np.int64)] >= thr) & \
            ~(occ[ri[w].astype(np.int64), rj[w].astype(np.int64)] >= thr)
        if free.all() and gaps(tx, ty) <= gap_lim and kappas(tx, ty) <= kap_lim:
            blend, bx, by = lam, tx, ty
            break
    out = dict(blend=blend, status=0, x0=np.stack([x0, y0], 1), xs=np.stack([xs, ys], 1), fixed=fx)
    if blend == 0:
        out.update(path=path.copy(), curvature=curv.copy())
        return out
    # grid -> world; fixed points keep their input bits
    ax, ay = bx - gx0, by - gy0
    xr = (ax * rc + ay * rs) + wgx
    yr = (-ax * rs + ay * rc) + wgy
    wx = np.where(fx, path[:, 0], xr).astype(np.float32)
    wy = np.where(fx, path[:, 1], yr).astype(np.float32)
    h = path[:, 2].copy()
    hh = np.arctan2(wy[i - 1] - wy[i + 1], wx[i - 1] - wx[i + 1]).astype(np.float32)
    if dirs is not None:
        rev = np.asarray(dirs, np.int8)[i] < 0
        hh = np.where(rev, np.where(hh > 0, hh - PI_F, hh + PI_F), hh).astype(np.float32)
    h[i] = hh
    k = np.arange(n)
    k[0], k[-1] = 1, n - 2
    kc = _menger(wx[k - 1], wy[k - 1], wx[k], wy[k], wx[k + 1], wy[k + 1])
    out.update(path=np.stack([wx, wy, h], 1).astype(np.float32), curvature=kc)
    return out


# ------------------------------------------------------------ float64 figures ----
def sum_second_diff2(path):
    """sum |x[i-1] - 2 x[i] + x[i+1]|^2 over the interior points, in float64."""
    p = np.asarray(path, np.float64)[:, :2]
    d = p[:-2] - 2 * p[1:-1] + p[2:]
    return float((d * d).sum())


def clearance64(xy, d2, res, d_max):
    """The bilinear clearance c(x) of grid-frame points, in float64 (indices clamped)."""
    xy = np.asarray(xy, np.float64)
    N = d2.shape[0]
    cell = np.where(d2 == CLEAR_NONE, float(d_max), float(res) * np.sqrt(np.where(d2 == CLEAR_NONE, 0, d2).astype(np.float64)))
    u, v = xy[:, 0] / float(res), xy[:, 1] / float(res)
    fi, fj = np.floor(u), np.floor(v)
    fu, fv = u - fi, v - fj
    cl = lambda a: np.clip(a, 0, N - 1).astype(np.int64)  # noqa: E731
    i0, i1, j0, j1 = cl(fi), cl(fi + 1), cl(fj), cl(fj + 1)
    a0 = cell[i0, j0] + fv * (cell[i0, j1] - cell[i0, j0])
    a1 = cell[i1, j0] + fv * (cell[i1, j1] - cell[i1, j0])
    return a0 + fu * (a1 - a0)


def objective(xy, xy0, d2, res, w_smooth=1.0, w_obs=0.5, w_fid=0.05, d_max=2.0):
    """J = w_smooth S + w_obs O + w_fid F of grid-frame points xy against the input xy0, in float64."""
    xy, xy0 = np.asarray(xy, np.float64), np.asarray(xy0, np.float64)
    c = clearance64(xy, d2, res, d_max)
    pen = np.where(c < d_max, d_max - c, 0.0)
    return float(w_smooth * sum_second_diff2(xy) + w_obs * (pen * pen).sum() + w_fid * ((xy - xy0) ** 2).sum())
