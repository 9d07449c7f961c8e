"""Step-by-step audit of a path a search returned (numpy, float64, no GPU).

A returned path is a certificate: a chain of motion-table primitives from the start pose, then
optionally one analytic shot (Dubins, or Reeds-Shepp with the reversing model) to the goal pose.
audit() re-derives every step from the planner's own tables and map and re-adds the cost, so a
path the vehicle model cannot drive, or a cost that is not the cost of the path handed back,
fails -- whichever search produced it.  It reads nothing of the search but its result; the chain /
shot split cannot be recovered from the poses (any suffix of a Dubins path resamples to itself), so
the caller passes it (`shot_len`: HybridAStar.shot_len() / OraclePlanner.find_path()["shot_len"]).

What is restated (oracle/hastar_oracle.cpp; csrc/hastar_relaxed.hip for the reversing model):
  start node   Planner::find_path: ci = nsteer / 2, vmin = vel^2, forward; pose (0, 0, 0) of the
               grid frame for a start outside the grid
  chain step   Planner::expand: child = parent + off[a][bin(h_p)], h_c = wrap(h_p + dth[a]), a in
               the steering window [max(ci_p - na, 0), .. + 2 na]; with vmin_p >= 1 the lateral
               limit vmin_p * curv_abs[a] <= a_lat and vmin_c = vmin_p - 2 sqrt(1 - lat^2 / a_lat^2) ts,
               else vmin_c = 0; the child's truncated cell is free; g += cost[a] + field(child)
  reverse step relaxed_expand: child = parent - off[a][bin(h_c)], h_c = wrap(h_p - dth[a]);
               cost[a] x rev_cost; gear_cost when the direction differs from the parent's
  shot         terminal = the shooter's parent, sample 0 stands for the shooter, cost = g(shooter) +
               the shot's cost (Dubins length; rs_cost for Reeds-Shepp)

Tolerances.  The three MEASURED_* values are the worst errors of this audit on the ORACLE's exact
paths (the reference for "a correct path audits this well"), never on the code under test;
measured by
    pytest tests/test_path_audit.py -s -k measured
on the cases of tests/test_path_audit.py:CASES.  TOL_POS and TOL_COST are 16 x the worst measured.
An off-by-one primitive is >= 0.1 m away and the smallest accounting error worth catching (one
mis-split step) is about 3e-5 of the cost, so TOL_COST must stay below 1e-5.
"""
import math

import numpy as np

MEASURED_MATCH_ERR = 1.91e-5   # worst chain-step error against its table primitive (m; rad for headings): synthetic512-1
MEASURED_SHOT_ERR = 5.6e-6     # worst shot-sample error against the regenerated Dubins shot: harness
MEASURED_COST_ERR = 1.07e-7    # worst |audited cost - reported cost| / reported cost: synthetic256-1
TOL_POS = 16 * max(MEASURED_MATCH_ERR, MEASURED_SHOT_ERR)
TOL_COST = 16 * MEASURED_COST_ERR
assert TOL_COST < 1e-5 and TOL_POS < 0.01
# Reeds-Shepp shots have no oracle search to measure on; the device's float solution is compared
# with the double-precision restatement at the tolerance tests/test_gpu_relaxed.py::
# test_reeds_shepp_device_matches_restatement uses for the same comparison
RS_REL, RS_ABS = 2e-4, 2e-3
BIN_EPS = 1e-5  # a heading this close to a bin boundary may round either way: both bins are tried


def wrap(a):
    """common.h wrap_pi: fmod, then fold into [-pi, pi]."""
    w = math.fmod(a, 2 * math.pi)
    if w > math.pi:
        return w - 2 * math.pi
    if w < -math.pi:
        return w + 2 * math.pi
    return w


def hdiff(a, b):
    """|a - b| as an angle."""
    return abs(math.remainder(a - b, 2 * math.pi))


def heading_bin(h, prec):
    """common.h heading index as the float planner computes it: round(h / prec) * prec is a float
    product, the rest is double arithmetic truncated -- so the rounding of that one product decides
    bins whose quotient is an integer (it is for every bin), and has to be restated, not idealised."""
    p = np.float32(prec)
    r = np.float32(np.float32(math.floor(abs(h) / float(p) + 0.5) * (1 if h >= 0 else -1)) * p)
    return int((float(r) + math.pi) / float(p))


def _bins(h, prec):
    out = []
    for e in (0.0, -BIN_EPS, BIN_EPS):
        for v in (h + e, wrap(h + e)):
            b = heading_bin(v, prec)
            if b not in out:
                out.append(b)
    return out


class Frame:
    """The planner's grid frame (Planner::update_goal / find_path), in float64."""

    def __init__(self, cfg, goal, frame_start):
        v = cfg.values
        self.N, self.res = v["grid_size"], float(np.float32(v["grid_resolution"]))
        self.n45, self.n2 = int(round(self.N * 0.8)), int(round(self.N * 0.5))
        self.goal = [float(np.float32(x)) for x in goal]
        fs = [float(np.float32(x)) for x in frame_start]
        self.gh = math.atan2(self.goal[1] - fs[1], self.goal[0] - fs[0])
        self.c, self.s = math.cos(self.gh), math.sin(self.gh)
        self.goal_pose = (self.n45 * self.res, self.n2 * self.res, wrap(self.goal[2] - self.gh))

    def to_grid(self, xyh):
        p = np.asarray(xyh, np.float64).reshape(-1, 3)
        dx, dy = p[:, 0] - self.goal[0], p[:, 1] - self.goal[1]
        out = np.empty_like(p)
        out[:, 0] = self.c * dx + self.s * dy + self.n45 * self.res
        out[:, 1] = -self.s * dx + self.c * dy + self.n2 * self.res
        out[:, 2] = [wrap(h - self.gh) for h in p[:, 2]]
        return out

    def inside(self, i, j):
        return -1 < i < self.N and -1 < j < self.N


def _cells(x, y, res, tol, rounding):
    """The cell of (x, y) -- truncated (successors) or rounded (shot samples) -- and those a
    position error of tol could move it to.  A coordinate that is a whole number of cells exactly
    (a start on a cell border in an unrotated frame, and every pose straight ahead of it) was
    recovered exactly: it gets its own cell only."""
    def axis(c):
        idx = []
        for e in ((0.0,) if c / res == math.floor(c / res) else (0.0, -tol, tol)):
            u = (c + e) / res
            i = int(math.floor(abs(u) + 0.5) * (1 if u >= 0 else -1)) if rounding else int(u)
            if i not in idx:
                idx.append(i)
        return idx
    return [(i, j) for i in axis(x) for j in axis(y)]


def _free(fr, occ, thr, x, y, tol, rounding):
    return any(fr.inside(i, j) and occ[i, j] < thr for i, j in _cells(x, y, fr.res, tol, rounding))


def audit(result, shot_len, planner_like, cfg, proto, *, mode, rev_cost=0.0, gear_cost=0.0, directions=None,
          frame_start=None, tol_pos=TOL_POS, tol_cost=TOL_COST):
    """Audit `result` (dict: path goal -> start in the world frame, curvature, cost) of a search from
    proto["start"] at proto["vel"] to proto["goal"].  planner_like: an OraclePlanner driven to the
    same map (motion_tables, field, get_obstacles, min_radius).  mode: "exact" or "relaxed".
    frame_start: the start pose the grid frame was set with (update_goal), when it is not
    proto["start"].  Raises AssertionError naming the failing pose index; returns a record."""
    from oracle import pyoracle, reeds_shepp as rs
    assert mode in ("exact", "relaxed")
    rev = rev_cost > 0.0
    assert not rev or mode == "relaxed", "the exact mode has no reversing model"
    assert not rev or directions is not None, "the reversing model's audit needs the direction flags"
    path = np.asarray(result["path"], np.float64)
    curv = np.asarray(result["curvature"])
    n, D = len(path), int(shot_len)
    assert result["ok"] and n >= 2 and len(curv) == n, f"no path to audit (ok={result['ok']}, {n} poses)"
    assert 0 <= D <= n, f"shot_len {D} of a path of {n} poses"
    assert D != 1, "a shot has at least its shooter and its end"
    if directions is not None:
        directions = np.asarray(directions)
        assert len(directions) == n and set(np.unique(directions).tolist()) <= {-1, 1}, "direction flags"
        assert rev or (directions == 1).all(), "reverse flags without the reversing model"
    assert (np.abs(path[:, 2]) <= math.pi + 1e-5).all(), "heading not wrapped"

    v = cfg.values
    fr = Frame(cfg, proto["goal"], frame_start if frame_start is not None else proto["start"])
    res = fr.res
    thr = np.float32(math.log(v["obstacle_threshold"] / (1.0 - v["obstacle_threshold"])))
    occ = planner_like.get_obstacles()
    mt = planner_like.motion_tables()
    off = mt["offsets"].astype(np.float64)
    dth = mt["dtheta"].astype(np.float64)
    acost = mt["cost"].astype(np.float64)
    cabs = mt["curv_abs"]
    prec = float(mt["precision"])
    nsteer, na = len(dth), v["num_actions"]
    ts, a_lat = np.float32(v["step_size"]), np.float32(v["max_lat_acc"])
    a_lat2 = np.float32(a_lat * a_lat)
    r_min = float(planner_like.min_radius())
    step = float(np.float32(v["step_size"]))
    G = fr.to_grid(path)

    rec = dict(kind="goal_node" if D == 0 else ("rs_shot" if rev else "forward_shot"), poses=n, shot_len=D,
               match_err=0.0, shot_err=0.0, actions=[], reverse_steps=0, gear_changes=0, shot_reverse=False,
               shooter_on_path=True)

    # ---- the start node
    s_grid = fr.to_grid(np.asarray([float(np.float32(x)) for x in proto["start"]]))[0]
    if not fr.inside(int(s_grid[0] / res), int(s_grid[1] / res)):
        s_grid = np.zeros(3)
    e0 = max(math.hypot(G[-1, 0] - s_grid[0], G[-1, 1] - s_grid[1]), hdiff(G[-1, 2], s_grid[2]))
    if D < n or rev:  # (a path that is all Dubins shot has the start as its shooter: checked below)
        assert e0 <= tol_pos, f"pose {n - 1}: not the start pose (off by {e0:.3g})"
        rec["match_err"] = max(rec["match_err"], e0)
    vel = np.float32(proto["vel"])
    st = dict(x=s_grid[0], y=s_grid[1], h=s_grid[2], ci=nsteer // 2, vmin=np.float32(vel * vel), dir=1)
    fields_at, step_costs = [], []

    def candidates(st):
        """(a, reverse, child pose, vmin_c) of every primitive expand() would try from st."""
        lo = max(st["ci"] - na, 0)
        out = []
        for a in range(lo, min(lo + 2 * na + 1, nsteer)):
            vm = np.float32(0.0)
            if not st["vmin"] < np.float32(1.0):
                lat = np.float32(st["vmin"] * cabs[a])
                if lat > a_lat:
                    continue
                al = np.float32(math.sqrt(1.0 - float(np.float32(np.float32(lat * lat) / a_lat2))))
                vm = np.float32(st["vmin"] - np.float32(np.float32(np.float32(2.0) * al) * ts))
            hc = wrap(st["h"] + dth[a])
            for b in _bins(st["h"], prec):
                out.append((a, False, (st["x"] + off[a, b, 0], st["y"] + off[a, b, 1], hc), vm))
            if rev:
                hr = wrap(st["h"] - dth[a])
                for b in _bins(hr, prec):
                    out.append((a, True, (st["x"] - off[a, b, 0], st["y"] - off[a, b, 1], hr), vm))
        return out

    def take(st, a, back, pose, vm, k, child_pose):
        """Account the step and return the child's state; child_pose: where the field is read."""
        d = -1 if back else 1
        if directions is not None:
            assert directions[k] == d, f"pose {k}: direction flag {directions[k]} on a {'reverse' if back else 'forward'} step"
        assert _free(fr, occ, thr, child_pose[0], child_pose[1], tol_pos, False), \
            f"pose {k}: the successor's cell is outside the grid or occupied"
        c = acost[a] * (rev_cost if back else 1.0) + (gear_cost if d != st["dir"] else 0.0)
        step_costs.append(c)
        fields_at.append(child_pose)
        rec["actions"].append((a, back))
        rec["reverse_steps"] += int(back)
        rec["gear_changes"] += int(d != st["dir"])
        return dict(x=child_pose[0], y=child_pose[1], h=child_pose[2], ci=a, vmin=vm, dir=d)

    def match(st, k, use_curv):
        """The one primitive that leads from st to pose k."""
        tgt = G[k]
        hits = []
        for a, back, p, vm in candidates(st):
            e = max(math.hypot(p[0] - tgt[0], p[1] - tgt[1]), hdiff(p[2], tgt[2]))
            if e <= tol_pos and not any(h[0] == a and h[1] == back for h in hits):
                hits.append((a, back, p, vm, e))
        lo = max(st["ci"] - na, 0)
        assert hits, (f"pose {k}: no motion primitive of the steering window [{lo}, {min(lo + 2 * na, nsteer - 1)}] "
                      f"(lateral limit applied: vmin {float(st['vmin']):.3f}) leads here from pose {k + 1}")
        if len(hits) > 1 and use_curv:
            same = [h for h in hits if cabs[h[0]] == curv[k + 1]]
            hits = same or hits
        if len(hits) > 1 and directions is not None:
            same = [h for h in hits if (-1 if h[1] else 1) == directions[k]]
            hits = same or hits
        costs = {round(acost[h[0]] * (rev_cost if h[1] else 1.0) + (gear_cost if (-1 if h[1] else 1) != st["dir"] else 0.0), 9)
                 for h in hits}
        assert len(costs) == 1, f"pose {k}: ambiguous step, primitives {[(h[0], h[1]) for h in hits]} with costs {sorted(costs)}"
        a, back, p, vm, e = hits[0]
        if use_curv:
            assert cabs[a] == curv[k + 1], f"pose {k}: curvature entry {curv[k + 1]} but action {a} has {cabs[a]}"
        rec["match_err"] = max(rec["match_err"], e)
        return a, back, p, vm

    # ---- the chain, from the start end
    stop = D if D > 0 else 0
    for k in range(n - 2, stop - 1, -1):
        a, back, p, vm = match(st, k, True)
        st = take(st, a, back, p, vm, k, tuple(G[k]))

    # ---- the terminal
    gp = fr.goal_pose
    shot_cost = 0.0
    if D == 0:
        assert (int(G[0, 0] / res), int(G[0, 1] / res)) == (fr.n45, fr.n2), "pose 0: not in the goal cell"
    elif not rev:
        # forward: the shooter is a successor of pose D (or the start); its Dubins shot, sampled as
        # the search samples it, must be the head of the path.  (Sample 0 is the shooter's pose
        # unless the first arc is shorter than one sample step -- then the shot starts at its
        # tangent point -- so the shooter is found as the successor whose shot reproduces the head.)
        if D < n:
            cands = [(a, p, vm) for a, back, p, vm in candidates(st)]
        else:
            cands = [(None, (st["x"], st["y"], st["h"]), st["vmin"])]
        found, why = [], []
        for a, p, vm in cands:
            sx, sc, length, flag = pyoracle.dubins_path_f(r_min, step, np.float32(p), np.float32(gp))
            if len(sx) != D:
                why.append(f"action {a}: {len(sx)} samples")
                continue
            sg = sx[::-1].astype(np.float64)
            e = max(float(np.hypot(sg[:, 0] - G[:D, 0], sg[:, 1] - G[:D, 1]).max()),
                    max(hdiff(x, y) for x, y in zip(sg[:, 2], G[:D, 2])))
            if e > tol_pos:
                why.append(f"action {a}: samples off by {e:.3g}")
                continue
            found.append((a, p, vm, sx, sc, length, flag, e))
        assert found, f"poses 0..{D - 1}: not the Dubins shot of any successor of pose {D} ({'; '.join(why)})"
        assert len(found) == 1, f"poses 0..{D - 1}: the shot of several successors {[f[0] for f in found]}"
        a, p, vm, sx, sc, length, flag, e = found[0]
        rec["shot_err"] = e
        assert not flag, "the shot's first arc is longer than 90 degrees: the search must not take it"
        assert (sc[::-1] == curv[1:D + 1]).all(), f"poses 0..{D - 1}: curvature entries differ from the shot's"
        for q in range(D):
            assert _free(fr, occ, thr, float(sx[q, 0]), float(sx[q, 1]), tol_pos, True), f"pose {D - 1 - q}: shot sample on an occupied cell"
        if a is not None:
            on = math.hypot(p[0] - G[D - 1, 0], p[1] - G[D - 1, 1]) <= tol_pos and hdiff(p[2], G[D - 1, 2]) <= tol_pos
            rec["shooter_on_path"] = on
            if on:
                rec["match_err"] = max(rec["match_err"], math.hypot(p[0] - G[D - 1, 0], p[1] - G[D - 1, 1]), hdiff(p[2], G[D - 1, 2]))
            st = take(st, a, False, p, vm, D - 1, p)
        shot_cost = float(length)
    else:
        if D < n:
            a, back, p, vm = match(st, D - 1, False)
            st = take(st, a, back, p, vm, D - 1, tuple(G[D - 1]))
        shot_cost = _audit_rs_shot(G, curv, directions, D, st, gp, r_min, step, rev_cost, gear_cost, fr, occ, thr, tol_pos, rec, rs)
    if D > 0 and mode == "relaxed":
        assert st["vmin"] < np.float32(1.0), f"pose {D - 1}: the shooter's vmin {float(st['vmin']):.3f} >= 1 allows no shot"

    # ---- the cost
    fld = planner_like.field(np.asarray(fields_at, np.float32)) if fields_at else np.zeros(0, np.float32)
    total = float(np.sum(step_costs)) + float(np.sum(fld.astype(np.float64))) + shot_cost
    rec.update(cost_audit=total, cost=float(result["cost"]), shot_cost=shot_cost,
               cost_err=abs(total - float(result["cost"])) / float(result["cost"]))
    assert rec["cost_err"] <= tol_cost, (f"cost: the path costs {total:.9g} ({len(step_costs)} steps + shot {shot_cost:.9g}) "
                                         f"but {result['cost']:.9g} was reported (relative {rec['cost_err']:.3g})")
    return rec


def _audit_rs_shot(G, curv, directions, D, st, gp, r, step, rev_cost, gear_cost, fr, occ, thr, tol, rec, rs):
    """The Reeds-Shepp shot of poses D - 1 (the shooter, sample 0) .. 0: returns its cost."""
    S = G[:D][::-1]                       # sample i = pose D - 1 - i
    sdir = directions[:D][::-1]           # sample i >= 1: the direction of travel that reached it
    skap = curv[1:D + 1][::-1]            # sample i >= 1: its segment's |curvature|
    kr = np.float32(1.0) / np.float32(r)
    segs = []                             # [turn (+1 L, 0 S, -1 R), dir, [per-sample arc lengths]]
    for i in range(1, D):
        k = D - 1 - i
        d = int(sdir[i])
        dh = math.remainder(S[i, 2] - S[i - 1, 2], 2 * math.pi)
        chord = math.hypot(S[i, 0] - S[i - 1, 0], S[i, 1] - S[i - 1, 1])
        if skap[i] == 0:
            assert abs(dh) <= tol, f"pose {k}: heading changes by {dh:.3g} on a straight sample"
            turn, ln = 0, chord
        else:
            assert abs(float(skap[i]) - float(kr)) <= 1e-6 * float(kr), f"pose {k}: curvature {skap[i]} is neither 0 nor 1 / r_min"
            turn = (1 if dh > 0 else -1) * d if abs(dh) > 1e-6 else None
            ln = abs(dh) * r
        assert ln <= step + tol, f"pose {k}: {ln:.4f} m of arc from the sample before, more than a step"
        if segs and segs[-1][1] == d and (turn is None and segs[-1][0] != 0 or segs[-1][0] == turn):
            segs[-1][2].append(ln)
        else:
            segs.append([1 if turn is None else turn, d, [ln]])
    assert 1 <= len(segs) <= 5, f"poses 0..{D - 1}: {len(segs)} segments, a Reeds-Shepp word has 1 to 5"
    # every sample lies on the curve integrated from the shooter with those segments
    x, y, h = st["x"], st["y"], st["h"]
    i, worst = 1, 0.0
    for turn, d, lens in segs:
        t = 0.0
        for ln in lens:
            t += d * ln
            if turn == 0:
                px, py, ph = x + t * math.cos(h), y + t * math.sin(h), h
            else:
                a = turn * t / r
                px = x + turn * r * (math.sin(h + a) - math.sin(h))
                py = y - turn * r * (math.cos(h + a) - math.cos(h))
                ph = h + a
            e = max(math.hypot(px - S[i, 0], py - S[i, 1]), hdiff(ph, S[i, 2]))
            assert e <= tol, f"pose {D - 1 - i}: off its segment's curve by {e:.3g}"
            worst = max(worst, e)
            assert _free(fr, occ, thr, S[i, 0], S[i, 1], tol, True), f"pose {D - 1 - i}: shot sample on an occupied cell"
            i += 1
        x, y, h = px, py, ph
    rec["shot_err"] = worst
    dist = math.hypot(gp[0] - st["x"], gp[1] - st["y"])
    eg = max(math.hypot(S[-1, 0] - gp[0], S[-1, 1] - gp[1]) / r, hdiff(S[-1, 2], gp[2]))
    assert eg < RS_ABS * max(1.0, dist / r), f"pose 0: the shot ends {eg:.3g} radii from the goal pose"
    fwd = sum(sum(l) for t, d, l in segs if d > 0)
    bwd = sum(sum(l) for t, d, l in segs if d < 0)
    ref = rs.length((st["x"], st["y"], st["h"]), gp, r)
    assert abs(fwd + bwd - ref) <= max(RS_REL * ref, RS_ABS), \
        f"poses 0..{D - 1}: a word of {fwd + bwd:.6f} m, the shortest is {ref:.6f} m"
    gears, d0 = 0, st["dir"]
    for t, d, l in segs:
        gears += int(d != d0)
        d0 = d
    rec["shot_reverse"] = bwd > 0
    rec["shot_segments"] = [(t, d, sum(l)) for t, d, l in segs]
    return fwd + rev_cost * bwd + gear_cost * gears
