"""Host statement of the sensor's fan geometry (numpy only; the device writes the same tables itself, ``fo_scene_fan``): class bits,
ray fan, the reference's footprint polygon and its range per ray, the half fan of the occluded area, the road union's holes."""
import numpy as np

from .scenario import MapGeometry

ROAD, VISIBLE, OCCLUDED = 1, 2, 4  # cell class bits (include/fo_hip.h)


def ray_dirs(n_rays, ego_yaw=0.0, fov_deg=360.0):
    """Unit ray directions, counter-clockwise.  Full circle (sensor_angle >= 359.9, sensor_model.py:121-122):
    angle_i = yaw + 2 pi i / n; open fan: n rays from yaw - fov/2 to yaw + fov/2 inclusive (:115-124)."""
    if fov_deg >= 359.9:
        ang = ego_yaw + 2.0 * np.pi * np.arange(n_rays) / n_rays
    else:
        half = np.radians(fov_deg) / 2.0
        ang = ego_yaw + np.linspace(-half, half, n_rays)
    return np.stack((np.cos(ang), np.sin(ang)), -1)


def footprint_ranges(n_rays, ego_yaw, fov_deg, r):
    """Range of the reference's sensor footprint along each ray of ``ray_dirs``.  The footprint is a polygon
    inscribed in the circle: ``Point(ego).buffer(r)`` = regular 64-gon with a vertex at world angle 0
    (sensor_model.py:121-122; shapely's default of 16 segments per quarter circle [ext]) for a full-circle sensor,
    else ego + 100 arc points (``_calc_relevant_sector``, :201-209).  Along direction phi the chord between two
    neighbouring arc points (angular pitch d) is met at r cos(d/2) / cos((phi - a0) mod d - d/2)."""
    if fov_deg >= 359.9:
        d = 2.0 * np.pi / 64.0
        rel = ego_yaw + 2.0 * np.pi * np.arange(n_rays) / n_rays
    else:
        d = np.radians(fov_deg) / 99.0
        rel = np.linspace(0.0, np.radians(fov_deg), n_rays)
    m = np.mod(rel, d)
    return r * np.cos(0.5 * d) / np.cos(m - 0.5 * d)


def half_fan_dirs(ego_yaw):
    """unit directions of the 100-point half fan about the heading; times 1.5 r they are the arc points of the polygon
    that bounds the reference's occluded area (sensor_model.py:85-87, 201-209)"""
    ang = np.linspace(ego_yaw - 0.5 * np.pi, ego_yaw + 0.5 * np.pi, 100)
    return np.stack((np.cos(ang), np.sin(ang)), -1)


def footprint_polygon(ego, yaw, fov_deg, r):
    """vertices of that polygon [n,2]"""
    if fov_deg >= 359.9:
        ang = np.arange(64) * (2.0 * np.pi / 64.0)
        return np.stack((ego[0] + r * np.cos(ang), ego[1] + r * np.sin(ang)), -1)
    half = np.radians(fov_deg) / 2.0
    ang = np.linspace(yaw - half, yaw + half, 100)
    arc = np.stack((ego[0] + r * np.cos(ang), ego[1] + r * np.sin(ang)), -1)
    return np.concatenate((np.asarray(ego, dtype=np.float64)[None], arc), axis=0)


class HoleIndex:
    """Interior rings (holes) of the road union's boundary and the per-step test "does the sensor footprint enclose
    this ring".  An enclosed ring is an interior ring of road ∩ footprint and casts no shadow in the reference, which
    walks `visible_area.exterior` only (sensor_model.py:126-131); a ring the footprint cuts open lies on the exterior
    of road ∩ footprint and does."""

    def __init__(self, geo: MapGeometry):
        self.edge_ring = np.asarray(geo.edge_ring)
        self.holes = []
        for k, pts in geo.holes():
            self.holes.append((k, pts))
        self.centres = np.array([pts.mean(axis=0) for _, pts in self.holes]).reshape(-1, 2)
        self.radii = np.array([float(np.sqrt(((pts - pts.mean(axis=0)) ** 2).sum(axis=1).max())) for _, pts in self.holes])

    def enclosed(self, ego_pos, ego_yaw, fov_deg, r, footprint="polygon"):
        """ids of the enclosed rings (all end points inside the footprint).  Cheap rejection first: the farthest
        vertex of a ring is at least as far from the ego as the ring's centroid."""
        if not self.holes:
            return ()
        ex, ey = float(ego_pos[0]), float(ego_pos[1])
        dx, dy = self.centres[:, 0] - ex, self.centres[:, 1] - ey
        near = dx * dx + dy * dy <= r * r
        if not near.any():                      # the usual case: one comparison per ring, no further work
            return ()
        ego = np.array([ex, ey])
        cand = np.nonzero(near & (self.radii <= 2.0 * r))[0]
        if len(cand) == 0:
            return ()
        from .scenario import points_in_polygon
        full = fov_deg >= 359.9
        foot = footprint_polygon(ego, ego_yaw, fov_deg, r) if not full else None
        out = []
        for i in cand:
            k, pts = self.holes[i]
            rho = np.hypot(pts[:, 0] - ego[0], pts[:, 1] - ego[1])
            inside = (rho <= r).all()
            if inside and full and footprint == "polygon":
                # inside the regular 64-gon Point(ego).buffer(r) (a vertex at world angle 0): the distance along the
                # normal of the sector's side stays below the apothem -- a handful of vector operations instead of a
                # crossing-number pass over 64 edges
                delta = 2.0 * np.pi / 64.0
                phi = np.mod(np.arctan2(pts[:, 1] - ego[1], pts[:, 0] - ego[0]), delta)
                near_side = rho * np.cos(phi - 0.5 * delta) > r * np.cos(0.5 * delta) * (1.0 - 1e-9)
                if near_side.any():             # within a hair of the polygon's side: let the exact test decide
                    inside = points_in_polygon(pts, footprint_polygon(ego, ego_yaw, fov_deg, r)).all()
            elif inside and foot is not None:
                inside = points_in_polygon(pts, foot).all()
            if inside:
                out.append(k)
        return tuple(out)

    def edge_skip(self, rings):
        """byte per boundary piece: 1 = on one of `rings`"""
        return np.isin(self.edge_ring, np.array(rings, dtype=np.int64)).astype(np.uint8)
