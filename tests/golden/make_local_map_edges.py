#!/usr/bin/env python3
"""Generate tests/golden/local_map_edges.npz: the reference's own get_local_map_angular (simulator/env.py:570-628) on
constructed scenes that reach the corners of its arithmetic, for tests/test_local_map_cpu.py and the GPU tests.

    python tests/golden/make_local_map_edges.py [--reference PATH]

Imports make_golden.py's shims (gym / cv2 / rvo2 stand-ins, not reference code) and calls the reference method with a
stand-in `self` that holds only what it reads: scene.obstacle_vertices, the angular_map_* settings and
calculate_angular_map_distances.  Everything written is data: polygons, poses, settings and the reference's outputs.
Cases:
  level_corner  theta = 0, vertices level with a corner of the robot's box (ry = +0, x < 0: sector dim)
  pi_cut        a polygon straddling the +-pi cut behind the robot (wrapped spans, dropped past dim)
  half_span     poses where two points of one walk lie exactly dim / 2 sectors apart (the wrap test's tie)
  overlap       the robot's box overlapping an obstacle
  dim72         dim = 72 (the shipped configs' other value)
  raw           normalize = False
"""
import argparse
import json
import math
import os
import sys
from types import SimpleNamespace as NS

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden  # noqa: E402

PI = math.pi


def rect(x0, x1, y0, y1):
    """scene.py's vertex order: (xm + hx, ym + hy), (xm - hx, ym + hy), (xm - hx, ym - hy), (xm + hx, ym - hy)."""
    return [[x1, y1], [x0, y1], [x0, y0], [x1, y0]]


def half_span_poses(vertices, dim, rs, want):
    """Random poses near a thin wall at which some (vertex, corner) pair of one walk set lies exactly dim / 2 apart."""
    res = 2 * PI / dim
    out = []
    for _ in range(200000):
        px, py, theta = rs.uniform(-0.6, 0.6), rs.uniform(-0.3, 0.3), rs.uniform(-PI, PI)
        r = 0.3
        c, s = np.cos(theta), np.sin(theta)
        corners = [(px + a * r, py + b * r) for a, b in ((-1, -1), (1, -1), (-1, 1), (1, 1))]

        def sector(v, e):
            rx = (v[0] - e[0]) * c + (v[1] - e[1]) * s
            ry = (v[1] - e[1]) * c - (v[0] - e[0]) * s
            return int((math.atan2(ry, rx) + PI) / float(res))
        hit = False
        for poly in vertices:
            for e in corners:  # phase 1 sets
                sec = [sector(v, e) for v in poly]
                hit |= any(abs(sec[i] - sec[j]) == dim // 2 for i in range(4) for j in range(i))
            for v in poly:  # phase 2 sets
                sec = [sector(v, e) for e in corners]
                hit |= any(abs(sec[i] - sec[j]) == dim // 2 for i in range(4) for j in range(i))
        if hit:
            out.append([px, py, r, theta])
            if len(out) == want:
                break
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default="/root/reference")
    args = ap.parse_args()
    make_golden.install_shims()
    sys.path.insert(0, args.reference)
    from simulator.env import EntityBasedCollisionAvoidance as Env

    def ref_map(vertices, pose, dim, max_range, amin, amax, normalize):
        me = NS(scene=NS(obstacle_vertices=vertices), angular_map_max_range=max_range, angular_map_dim=dim,
                angular_map_min_angle=amin, angular_map_max_angle=amax, local_maps_angular=[])
        me.calculate_angular_map_distances = lambda *a: Env.calculate_angular_map_distances(me, *a)
        ob = NS(px=pose[0], py=pose[1], radius=pose[2], theta=pose[3])
        return np.array(Env.get_local_map_angular(me, ob, normalize=normalize, append=False))

    rs = np.random.RandomState(7)
    five = [rect(1.0, 1.5, -2.0, 1.0), rect(-2.5, -1.0, 0.5, 0.8), rect(-0.4, 0.4, 1.2, 2.2),
            rect(-3.0, -2.0, -3.0, -2.0), rect(2.0, 2.3, 2.0, 4.0)]
    wall = [rect(-2.0, 2.0, 0.45, 0.55)]
    cases = [
        ("level_corner", [rect(-2.0, -1.0, -0.3, 0.3), rect(1.0, 2.0, -0.3, 0.3), rect(-0.3, 0.3, 1.0, 2.0)],
         [[0.0, 0.0, 0.3, 0.0], [0.5, 0.0, 0.3, 0.0], [0.0, 1.3, 0.3, 0.0], [0.0, -0.7, 0.3, 0.0]], 48, 3.0, True),
        ("pi_cut", [rect(-2.0, -1.0, -0.5, 0.5), rect(-1.2, -0.6, -0.05, 0.07)],
         [[0.0, 0.05, 0.2, 0.0], [0.0, -0.02, 0.3, 0.0], [0.1, 0.0, 0.2, 1e-3], [0.0, 0.0, 0.2, -1e-3],
          [0.3, 0.2, 0.3, PI / 2], [0.0, 0.0, 0.2, PI]], 48, 3.0, True),
        ("half_span", wall, half_span_poses(wall, 48, rs, 8), 48, 3.0, True),
        ("overlap", [rect(-1.0, 1.0, -1.0, 1.0), rect(0.1, 0.4, -0.2, 2.0)],
         [[0.1, 0.2, 0.3, 0.7], [0.0, 0.0, 0.2, 0.0], [0.9, -0.9, 0.3, -2.5], [0.25, 0.5, 0.3, 2.0]], 48, 3.0, True),
        ("dim72", five, [[rs.uniform(-3, 3), rs.uniform(-3, 3), 0.3, rs.uniform(-PI, PI)] for _ in range(12)], 72, 3.0,
         True),
        ("raw", five, [[rs.uniform(-3, 3), rs.uniform(-3, 3), 0.2, rs.uniform(-PI, PI)] for _ in range(12)], 48, 3.0,
         False),
    ]
    out = {}
    for k, (name, vertices, poses, dim, max_range, normalize) in enumerate(cases):
        assert len(poses) > 0, name
        maps = [ref_map(vertices, p, dim, max_range, -PI, PI, normalize) for p in poses]
        out["pose_%d" % k] = np.array(poses, dtype=np.float64)
        out["map_%d" % k] = np.array(maps)
        out["meta_%d" % k] = make_golden.jdump({"name": name, "vertices": vertices, "max_range": max_range, "dim": dim,
                                                "angle_min": -PI, "angle_max": PI, "normalize": normalize})
    out["n"] = np.array(len(cases))
    np.savez_compressed(os.path.join(os.path.dirname(os.path.abspath(__file__)), "local_map_edges.npz"), **out)
    print("wrote local_map_edges.npz (%d cases)" % len(cases))


if __name__ == "__main__":
    main()
