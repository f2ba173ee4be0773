"""NumPy brute-force checker of the extended future-visibility sweep (fo_scene_future_visibility_ex): per pose the first
hit of every ray over all boundary pieces and the obstacles of the pose's occluder slice, the fan (full circle or open
sector, rotated by the given heading vectors), the chord rule over the occluded list and a seen set per trajectory.

The arithmetic restates the C oracle's (oracle/fo_oracle_scene.c: ray_segment, first_hit, fan_ccw / fan_search /
fan_sector, fo_oracle_future_visibility) element by element in float64; numpy evaluates every expression as written (no
contraction), so counts are exact and only the order of the area sum differs from a serial one."""
import numpy as np


def first_hits(ox, oy, dx, dy, segs, r):
    """ranges [n] of the rays (ox, oy) + t (dx, dy) against segs [S, 4] (ax, ay, bx, by): min t over hits, clamped to r"""
    ax, ay, bx, by = (segs[:, i][None, :] for i in range(4))
    dx, dy = dx[:, None], dy[:, None]
    ex, ey = bx - ax, by - ay
    denom = dx * ey - dy * ex
    wx, wy = ax - ox, ay - oy
    tn = wx * ey - wy * ex
    un = wx * dy - wy * dx
    pos = (tn >= 0.0) & (un >= 0.0) & (un <= denom)
    neg = (tn <= 0.0) & (un <= 0.0) & (un >= denom)
    hit = (denom != 0.0) & np.where(denom > 0.0, pos, neg)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(hit, tn / np.where(denom == 0.0, 1.0, denom), np.inf)
    best = t.min(axis=1) if t.shape[1] else np.full(t.shape[0], np.inf)
    return np.where(best <= r, best, r)


def obstacle_segments(ocorn, oflags):
    """the four sides of every present, occluding obstacle: [4 O', 4]"""
    ocorn = np.asarray(ocorn, dtype=np.float64).reshape(-1, 4, 2)
    keep = (np.asarray(oflags) & 1).astype(bool) & (np.asarray(oflags) & 2).astype(bool)
    c = ocorn[keep]
    if len(c) == 0:
        return np.zeros((0, 4))
    nxt = c[:, [1, 2, 3, 0]]
    return np.concatenate((c, nxt), axis=2).reshape(-1, 4)


def _ccw(dirs, i, rx, ry):
    n = len(dirs)
    d = dirs[np.where(i == n, 0, i)]
    c = d[:, 0] * ry - d[:, 1] * rx
    dot = d[:, 0] * rx + d[:, 1] * ry
    return np.where(c > 0.0, True, np.where(c < 0.0, False, dot > 0.0))


def _search(dirs, a, b, rx, ry):
    m = len(rx)
    lo, hi = np.full(m, a), np.full(m, b)
    ok = _ccw(dirs, lo, rx, ry) & ~_ccw(dirs, hi, rx, ry)
    while True:
        act = hi - lo > 1
        if not act.any():
            break
        mid = (lo + hi) >> 1
        c = _ccw(dirs, mid, rx, ry)
        lo = np.where(act & c, mid, lo)
        hi = np.where(act & ~c, mid, hi)
    return np.where(ok, lo, -1)


def fan_sector(dirs, full, rx, ry):
    """the i with (rx, ry) in [ray i, ray i + 1) counter-clockwise, -1 outside an open fan (fo_oracle_scene.c)"""
    n = len(dirs)
    if full:
        a, b = n // 3, (2 * n) // 3
        s = _search(dirs, 0, a, rx, ry)
        s = np.where(s >= 0, s, _search(dirs, a, b, rx, ry))
        return np.where(s >= 0, s, _search(dirs, b, n, rx, ry))
    m = (n - 1) // 2
    s = _search(dirs, 0, m, rx, ry)
    return np.where(s >= 0, s, _search(dirs, m, n - 1, rx, ry))


def pose_fan(dirs, heading):
    """the unit fan of one pose: dirs rotated by the heading vector (c, s) as the kernel does, or dirs (None)"""
    if heading is None:
        return dirs
    c, s = float(heading[0]), float(heading[1])
    ux, uy = dirs[:, 0], dirs[:, 1]
    return np.stack((c * ux - s * uy, s * ux + c * uy), -1)


def future_visibility(x, y, t_stride, dirs, r, edges, ocorn, oflags, occ_idx, rx0, ry0, cs, ix0, iy0, nx, full=True,
                      heading=None, rows=None):
    """(revealed [M', K] int32, area [M', K], revealed_new [M', K] int32, revealed_any [M'] int32) for the trajectories
    ``rows`` (default all).  ocorn [S, O, 4, 2] / oflags [S, O]: pose k casts against slice min(k, S - 1).  dirs: the
    unit fan about heading 0 (full circle when ``full``, else the open sector); heading [M, K, 2] or None."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    dirs = np.asarray(dirs, dtype=np.float64).reshape(-1, 2)
    edges = np.asarray(edges, dtype=np.float64).reshape(-1, 4)
    ocorn = np.asarray(ocorn, dtype=np.float64)
    oflags = np.asarray(oflags, dtype=np.uint8)
    S = ocorn.shape[0]
    segs = [np.concatenate((edges, obstacle_segments(ocorn[s], oflags[s])), axis=0) for s in range(S)]
    occ_idx = np.asarray(occ_idx, dtype=np.int64)
    wx, wy = ix0 + occ_idx % nx, iy0 + occ_idx // nx
    cx, cy = rx0 + (wx.astype(np.float64) + 0.5) * cs, ry0 + (wy.astype(np.float64) + 0.5) * cs
    M, T = x.shape
    K = (T + t_stride - 1) // t_stride
    rows = range(M) if rows is None else rows
    n = len(dirs)
    r2 = r * r
    out_rev, out_area, out_new, out_any = [], [], [], []
    for m in rows:
        seen = np.zeros(len(occ_idx), dtype=bool)
        rev, area, new = np.zeros(K, np.int32), np.zeros(K), np.zeros(K, np.int32)
        for k in range(K):
            px, py = x[m, k * t_stride], y[m, k * t_stride]
            d = pose_fan(dirs, None if heading is None else heading[m, k])
            sg = segs[min(k, S - 1)]
            # pieces farther than r from the pose cannot hit within r (their t would be clamped to r anyway)
            gx = np.maximum(np.maximum(np.minimum(sg[:, 0], sg[:, 2]) - px, px - np.maximum(sg[:, 0], sg[:, 2])), 0.0)
            gy = np.maximum(np.maximum(np.minimum(sg[:, 1], sg[:, 3]) - py, py - np.maximum(sg[:, 1], sg[:, 3])), 0.0)
            rng = first_hits(px, py, d[:, 0], d[:, 1], sg[gx * gx + gy * gy <= (r + 1e-6) ** 2], r)
            h = rng[:, None] * d
            j = np.arange(1, n + 1) % n
            terms = h[:, 0] * h[j, 1] - h[j, 0] * h[:, 1]
            if not full:
                terms = terms[:-1]
            a2 = 0.0
            for v in terms:
                a2 += v
            area[k] = 0.5 * a2
            qx, qy = cx - px, cy - py
            inside = np.zeros(len(occ_idx), dtype=bool)
            near = ~(qx * qx + qy * qy > r2)
            zero = near & (qx == 0.0) & (qy == 0.0)
            cand = near & ~zero
            if cand.any():
                qxc, qyc = qx[cand], qy[cand]
                i = fan_sector(d, full, qxc, qyc)
                ii = np.where(i < 0, 0, i)
                jj = np.where(ii + 1 == n, 0, ii + 1)
                hix, hiy, hjx, hjy = h[ii, 0], h[ii, 1], h[jj, 0], h[jj, 1]
                ok = (i >= 0) & ((hjx - hix) * (qyc - hiy) - (hjy - hiy) * (qxc - hix) >= 0.0)
                inside[cand] = ok
            inside |= zero
            rev[k] = int(inside.sum())
            new[k] = int((inside & ~seen).sum())
            seen |= inside
        out_rev.append(rev)
        out_area.append(area)
        out_new.append(new)
        out_any.append(int(new.sum()))
    return (np.array(out_rev, dtype=np.int32).reshape(-1, K), np.array(out_area).reshape(-1, K),
            np.array(out_new, dtype=np.int32).reshape(-1, K), np.array(out_any, dtype=np.int32))
