"""Shared by tests/test_crowd_rules_cpu.py and tests/test_crowd_rules_gpu.py: the reference's scenes under the crowd rules
(tests/golden/scenes_crowd_rules.npz, made by tests/golden/make_golden_crowd_rules.py) as padded batches, the mask of the
adults the circle rule placed, and the comparison bar of tests/test_scene_gen.py."""
import configparser
import copy
import json

import numpy as np

from ebcsim import scene as ebc_scene
from helpers import load
from test_scene_gen import ARRAYS, _compare_batches

RULES = ("mixed", "mixed_20", "one_static")
CAPACITY = {"mixed": 5, "mixed_20": 20, "one_static": 2}


def scene_config(text):
    cfg = configparser.RawConfigParser()
    cfg.read_string(text)
    return ebc_scene.SceneConfig.from_config(cfg)


def empty_batch(n, N, S, G):
    f = lambda *sh: np.zeros(sh)  # noqa: E731
    S1 = max(S, 1)
    return ebc_scene.SceneBatch(n, N, S, np.zeros(n, np.int32), f(n, N), f(n, N), f(n, N), f(n, N), f(n, N), f(n, N),
                                f(n, N), f(n, N), np.zeros((n, N), np.uint8), np.zeros(n, np.int32), f(n, S1), f(n, S1),
                                f(n, S1), np.zeros((n, G, 2), np.uint64), f(n, 9))


class GoldenSet:
    """One set of the fixture: the scenes of one config, as the reference generated them."""

    def __init__(self, z, s):
        self.meta = json.loads(str(z["meta_%d" % s]))
        self.rule, self.randomized, self.text = self.meta["rule"], self.meta["randomized"], self.meta["config_text"]
        self.cfg = scene_config(self.text)
        self.seeds = [int(v) for v in z["seed_%d" % s]]
        self.count, self.n_static = z["count_%d" % s], z["n_static_%d" % s]
        self._z, self._s = z, s
        self.tag = self.rule + ("/randomized" if self.randomized else "")

    def batch(self, pad_humans=1, pad_static=2):
        """The expected scenes as a SceneBatch with `pad_humans` free slots past the rule's capacity (and the other
        types' counts) and `pad_static` free static rows; the tails are zero."""
        z, s = self._z, self._s
        n = len(self.seeds)
        N = CAPACITY[self.rule] + self.cfg.bicycle_num + self.cfg.children_num + pad_humans
        S = int(self.n_static.max()) + pad_static if self.n_static.max() else 0
        grids = np.unpackbits(z["grid_%d" % s], axis=2)[:, :, :z["grid_%d" % s].shape[1]]  # 1 = occupied
        b = empty_batch(n, N, S, grids.shape[1])
        ho = np.concatenate([[0], np.cumsum(self.count)])
        so = np.concatenate([[0], np.cumsum(self.n_static)])
        for e in range(n):
            k, m = int(self.count[e]), int(self.n_static[e])
            b.n_humans[e], b.n_static[e] = k, m
            for key in ("px", "py", "vx", "vy", "gx", "gy", "radius", "v_pref", "type"):
                getattr(b, key)[e, :k] = z["%s_%d" % (key, s)][ho[e]:ho[e + 1]]
            if m:
                b.spx[e, :m], b.spy[e, :m], b.sradius[e, :m] = z["static_%d" % s].reshape(-1, 3)[so[e]:so[e + 1]].T
            b.grid[e] = ebc_scene.pack_grid(1.0 - grids[e])
            b.robot[e] = z["robot_%d" % s][e]
        return b


def golden_sets():
    z = load("scenes_crowd_rules")
    return [GoldenSet(z, s) for s in range(int(z["n_sets"]))]


def circle_mask(b):
    """Where the circle rule placed a human of batch `b`: the goal is the position mirrored (no other rule does that)."""
    live = np.arange(b.N)[None, :] < b.n_humans[:, None]
    return live & (b.gx == -b.px) & (b.gy == -b.py) & ((b.px != 0) | (b.py != 0))


def compare(got, want, tag, exact=False):
    """The bar of tests/test_scene_gen.py: every array bit for bit, but the positions and goals of circle-placed adults
    within 1 ulp.  Returns (values that differ, circle-placed values)."""
    circle = None if exact else circle_mask(want)
    if got.grid is None:  # a batch copied back from the device has no grid when no scene has an obstacle
        got.grid = np.zeros_like(want.grid)
    differ = _compare_batches(got, want, circle, tag)
    return differ, 0 if exact else 4 * int(circle.sum())


def with_rule(cfg, rule, randomized):
    """`cfg` with the adults on `rule`; with `randomized`, random attributes in the ranges of the randomised golden set."""
    c = copy.deepcopy(cfg)
    c.test_sim_adult = c.train_val_sim_adult = rule
    c.adult_num = CAPACITY[rule]
    c.randomize_attributes = randomized
    return c


__all__ = ["ARRAYS", "CAPACITY", "RULES", "GoldenSet", "circle_mask", "compare", "empty_batch", "golden_sets", "scene_config",
           "with_rule"]
