"""World-frame trajectories of an evaluation: what the reference keeps per step in env.states (simulator/env.py:344-351:
the robot's FullState and the humans' observable states before every step) for its trajectory plots and for a look at a
failed case, kept on the device for every env of a batch.

    rec = EpisodeRecorder(env, steps)
    m = train.evaluate(env, decide, gamma, record=rec)                      # per step: three gathers into the buffers
    m = train.evaluate_windows(env, rec.recording(rollout), gamma, K)       # per window: the rollout writes them itself
    ep = rec.episodes()      # host arrays, every env cut at its terminal step
    rec.save("episodes.npz")

Index t of a buffer is the state BEFORE step t, the convention of ebc_step_k's state_rotated[t]; an episode of `length`
steps has `length` records (the state its terminal step was taken from is the last; the state behind the terminal step is
not part of the reference's list either, which appends before it advances)."""
import numpy as np
import torch


class EpisodeRecorder(object):
    """Device buffers robot [steps, E, 9] float64, ob [steps, E, R, 5] float64 and n_rows [steps, E] int64 for one
    episode per env of `env` (a BatchedEnv on a HIP device), filled by train.evaluate / train.evaluate_windows."""

    def __init__(self, env, steps):
        dev = torch.device("cuda", env.device)
        steps, E, R = int(steps), env.E, env.R
        if steps < 1:
            raise ValueError("EpisodeRecorder: steps must be at least 1")
        self.env, self.steps, self.E, self.R = env, steps, E, R
        self.robot = torch.zeros((steps, E, 9), dtype=torch.float64, device=dev)
        self.ob = torch.zeros((steps, E, R, 5), dtype=torch.float64, device=dev)
        self.n_rows = torch.zeros((steps, E), dtype=torch.int64, device=dev)
        # the steps' own done flags and codes: where to cut, and how the episode ended
        self.done = torch.zeros((steps, E), dtype=torch.uint8, device=dev)
        self.info = torch.zeros((steps, E), dtype=torch.uint8, device=dev)
        self.filled = 0
        self.end_time = None  # the tally's end times, [E] on the host, where evaluate() handed its tally over
        # what does not change over an episode (no auto-reset in an evaluation): the humans' types, and the case an env holds
        self.type = env.get_state()["type"].copy()
        self.case = np.arange(E, dtype=np.int64)

    def _room(self, t0, k):
        if t0 + k > self.steps:
            raise ValueError("EpisodeRecorder: steps %d..%d do not fit the %d recorded steps" % (t0, t0 + k, self.steps))
        self.filled = max(self.filled, t0 + k)

    def before_step(self, t):
        """The per-step loop: the state before step t, by the three gathers collect_sail_demos uses."""
        self._room(t, 1)
        self.env.robot_state_device(self.robot[t])
        self.env.observe_ob_device(self.ob[t])
        self.env.row_counts_device(self.n_rows[t])

    def window_outputs(self, t0, k):
        """The window t0 .. t0 + k: the three outputs a rollout writes itself (ebc_step_k_world), as step_k_device takes
        them."""
        self._room(t0, k)
        return dict(world_robot=self.robot[t0:t0 + k], world_ob=self.ob[t0:t0 + k], n_rows=self.n_rows[t0:t0 + k])

    def recording(self, rollout):
        """rollout(env, K, outputs) as train.evaluate_windows calls it -> the same, with the window's world outputs added
        and its done / info kept; the windows follow one another from step 0 on."""
        def recorded(env, K, outputs):
            t0 = self.filled
            window = dict(outputs)
            window.update(self.window_outputs(t0, K))
            rollout(env, K, window)
            self.after_steps(t0, outputs["done"], outputs["info"])
        return recorded

    def after_steps(self, t0, done, info):
        """done and info, [E] or [k, E], of the steps from t0 on, as the step wrote them."""
        done, info = done.reshape(-1, self.E), info.reshape(-1, self.E)
        self.done[t0:t0 + done.shape[0]].copy_(done)
        self.info[t0:t0 + info.shape[0]].copy_(info)

    def finish(self, tally):
        self.end_time = tally.end_time.cpu().numpy()

    def episodes(self, tally=None):
        """Host arrays, every env cut at its first terminal step: robot [steps, E, 9], ob [steps, E, R, 5] and n_rows
        [steps, E] with zeros from index length[e] on, length [E] (the steps of the episode: its terminal step is step
        length - 1; the recorded steps when the env never ended), final [E] (the info code of the terminal step, what the
        evaluation's tally keeps as `final`; -1: the env never ended).  With `tally` (a train._EpisodeTally) its end
        signals are checked against the recorder's own."""
        n = self.filled
        done = self.done[:n].cpu().numpy() != 0
        ended = done.any(axis=0)
        last = done.argmax(axis=0)
        length = np.where(ended, last + 1, n).astype(np.int64)
        final = np.where(ended, self.info[:n].cpu().numpy().astype(np.int64)[last, np.arange(self.E)], -1)
        if tally is not None and not np.array_equal(final, tally.final.cpu().numpy()):
            raise ValueError("EpisodeRecorder: the tally's end signals are not those of the recorded steps")
        live = np.arange(self.steps)[:, None] < length[None, :]  # [steps, E]
        robot, ob, n_rows = self.robot.cpu().numpy(), self.ob.cpu().numpy(), self.n_rows.cpu().numpy()
        robot = np.where(live[:, :, None], robot, 0.0)
        ob = np.where(live[:, :, None, None], ob, 0.0)
        n_rows = np.where(live, n_rows, 0)
        return dict(robot=robot, ob=ob, n_rows=n_rows, length=length, final=final.astype(np.int64))

    def save(self, path, tally=None):
        """One .npz: episodes() plus the humans' `type` [E, N], the case index of every env and the time step."""
        ep = self.episodes(tally)
        with open(path, "wb") as f:  # a file object: numpy appends no suffix to the name
            np.savez_compressed(f, type=self.type, case=self.case, time_step=np.float64(self.env.params.time_step), **ep)
        return path
