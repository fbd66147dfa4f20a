"""Humans on a policy per entity type (EBC_HUMAN_BY_TYPE), by the checker as it stands: the rule of include/ebcsim.h at
ebc_set_human_policies composed from what oracle/ already has.  lookahead(one action, HUMAN_ORCA) leaves every human's
ORCA velocity in the checker's human_action, lookahead(HUMAN_LINEAR) the linear ones; each human takes its own type's, and
the step is the HUMAN_EXTERNAL step with exactly those doubles.  MixedOracle has BatchedEnv's call surface with
set_human_policies on it, so it also serves as the facade's injected backend."""
import configparser
import io
import json

import numpy as np

from ebcsim import _abi
from oracle import oracle

ORCA, LINEAR, BY_TYPE = _abi.HUMAN_ORCA, _abi.HUMAN_LINEAR, _abi.HUMAN_BY_TYPE
CODE = {"orca": ORCA, "linear": LINEAR}
ALL_TABLES = [(a, b, c) for a in (ORCA, LINEAR) for b in (ORCA, LINEAR) for c in (ORCA, LINEAR)]
BIKES_LINEAR, ADULTS_LINEAR = (ORCA, LINEAR, ORCA), (LINEAR, ORCA, LINEAR)
_ZERO_ACTION = np.zeros((1, 2))


class MixedOracle(oracle.OracleEnv):
    def __init__(self, params, n_envs, max_humans, max_static, library=None):
        oracle.OracleEnv.__init__(self, params, n_envs, max_humans, max_static, library)
        self.human_policies = (ORCA, ORCA, ORCA)

    def set_human_policies(self, adult, bicycle, child):
        table = (int(adult), int(bicycle), int(child))
        assert all(c in (ORCA, LINEAR) for c in table), table
        self.human_policies = table

    def mixed_velocities(self):
        """[E, N, 2]: each human's own policy's velocity from the current state."""
        oracle.OracleEnv.lookahead(self, _ZERO_ACTION, human_policy=ORCA, want_rows=False)
        orca = self.a["human_action"].copy()
        oracle.OracleEnv.lookahead(self, _ZERO_ACTION, human_policy=LINEAR, want_rows=False)
        linear = self.a["human_action"].copy()
        on_linear = np.array(self.human_policies + (ORCA,))[np.minimum(self.a["type"], 3)] == LINEAR
        return np.where(on_linear[..., None], linear, orca)

    def _humans(self, human_policy):
        if human_policy != BY_TYPE:
            return human_policy
        self.set_human_actions(self.mixed_velocities())
        return _abi.HUMAN_EXTERNAL

    def step(self, robot_action=None, human_policy=ORCA, robot_policy=_abi.ROBOT_EXTERNAL, flags=0, border=None):
        return oracle.OracleEnv.step(self, robot_action, self._humans(human_policy), robot_policy, flags, border)

    def lookahead(self, actions, human_policy=ORCA, flags=0, border=None, want_rows=True):
        # the velocities stay in human_action, where a following HUMAN_CACHED step reads them
        return oracle.OracleEnv.lookahead(self, actions, self._humans(human_policy), flags, border, want_rows)


class AsMixed(object):
    """An env whose step and lookahead run HUMAN_BY_TYPE whatever policy the caller names: lets helpers.check_trajectory,
    which reads one of orca / linear from a fixture's meta, replay a mixed fixture."""

    def __init__(self, env, table):
        self._env = env
        env.set_human_policies(*table)

    def __getattr__(self, name):
        return getattr(self._env, name)

    def step(self, robot_action=None, human_policy=None, **kw):
        return self._env.step(robot_action=robot_action, human_policy=BY_TYPE, **kw)

    def lookahead(self, actions, human_policy=None, **kw):
        return self._env.lookahead(actions, human_policy=BY_TYPE, **kw)


def table_of(z):
    """(adult, bicycle, child) codes from a mixed fixture's meta."""
    return tuple(CODE[name] for name in json.loads(str(z["meta"]))["human_policies"])


def config_text_of_mixed(z):
    """The INI text the mixed fixture ran with: the scenes fixture's text of its config file plus every recorded override,
    the per-type policies included."""
    from helpers import load
    meta = json.loads(str(z["meta"]))
    zs = load("scenes")
    for k in range(int(zs["n"])):
        m = json.loads(str(zs["meta_%d" % k]))
        if m["config"] == meta["config"]:
            cfg = configparser.RawConfigParser()
            cfg.read_string(m["config_text"])
            for key, val in meta["overrides"].items():
                sec, opt = key.split(".")
                cfg.set(sec, opt, str(val))
            buf = io.StringIO()
            cfg.write(buf)
            return buf.getvalue()
    raise KeyError(meta["config"])


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()
