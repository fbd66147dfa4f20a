#!/usr/bin/env python3
"""Per-wave timeline of the step kernels: when each one-wave workgroup started and ended, on the
device's constant 100 MHz clock, and how many shader cycles it lived.  Needs the trace build:

    make -C eb-cadrl_amd/csrc trace
    EBCSIM_LIB=eb-cadrl_amd/lib/libebcsim_trace.so python3 tools/wave_timeline.py [workload] [envs]

Prints, per kernel role: first/last start, last end (us from the first start of the launch),
wave lifetime percentiles, the shader clock the lifetimes imply, and how many waves were resident
over time.  With marks (make trace TRACE_LEVEL=2) also the roles' marks on the launch's time axis and the segments of
the heads of the ROWS and STATE waves: arguments staged, state back, then robot_ready seen and robot_n back (ROWS) or
restart scene back and restart robot parked (STATE, which that build waits for part by part), p10 / p50 / p90 and for the
six waves that stored last, over the waves that passed every mark of the head.
"""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "eb-cadrl_amd")):
    sys.path.insert(0, p)

TAGS = {0: "orca_kernel", 1: "step_kernel", 2: "orca_step_kernel", 3: "(unused)"}


def main():
    import numpy as np
    import torch
    import bench
    from ebcsim import _abi, _capi
    from ebcsim.batched import BatchedEnv
    workload = sys.argv[1] if len(sys.argv) > 1 else "metric"
    E = int(sys.argv[2]) if len(sys.argv) > 2 else bench.WORKLOADS[workload][2]
    L = _capi.lib()
    L.ebc_debug_wave_trace.restype = C.c_int
    L.ebc_debug_wave_trace.argtypes = [C.c_void_p, C.c_uint]
    params, batch = bench.build_batch(workload, E, 0)
    env = BatchedEnv(params, E, batch.N, batch.S)
    env.reset(batch)
    env.use_torch_stream()
    blocks = 1 << 17
    buf = torch.zeros((4, blocks, 16), dtype=torch.int64, device="cuda")
    _capi.check(L.ebc_debug_wave_trace(buf.data_ptr(), blocks))
    outs = env.alloc_step_outputs(("reward", "done", "info", "obs_rotated"))
    fl = _abi.FLAG_AUTO_RESET
    for hp in (_abi.HUMAN_LINEAR, _abi.HUMAN_ORCA):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        for i in range(60):
            if i == 10:
                ev[0].record()
            env.step_device(outs, human_policy=hp, robot_policy=_abi.ROBOT_LINEAR, flags=fl)
        ev[1].record()
        torch.cuda.synchronize()
        # the launch-to-launch period of THIS build, to set beside the last wave's end below: the difference is
        # what the launch spends before its first wave and after its last one (dispatch, end-of-kernel write-back)
        print("%s: %.2f us per step over 50 back-to-back launches (events)" % (
            "linear humans" if hp == _abi.HUMAN_LINEAR else "ORCA humans", ev[0].elapsed_time(ev[1]) * 1e3 / 50))
    t = buf.cpu().numpy().astype(np.uint64)
    launch0 = None
    for tag in (2, 3, 1):
        rows = t[tag]
        idx = np.nonzero(rows[:, 1] != 0)[0]
        rows = rows[idx]
        if not len(rows):
            continue
        if tag == 2:  # orca_step_kernel: blocks in role order ENV, ORCA, ROWS, STATE, each dealt to the eight classes
            # of envs by block index mod 8 (csrc/ebc_step_grid.h, restated)
            others = batch.N - 1 + (1 if params.robot_visible else 0)
            gs = next(g for g in (2, 3, 4, 5, 6, 7, 8, 9, 10, 12, 16, 21, 32) if g >= others)
            R = batch.N + batch.S
            grid = StepGrid(E, batch.N, 64 // gs, 64 // R if R <= 64 else 1)
            b1, b2, b3 = grid.base["ORCA"], grid.base["ROWS"], grid.base["STATE"]
            state_blocks = grid.blocks["STATE"]
            busy = np.zeros(grid.total, bool)  # blocks that own something: the others start and end at once
            for role in grid.base:
                busy[grid.base[role]:grid.base[role] + grid.blocks[role]] = grid.owns(np, role)
            own = busy[np.minimum(idx, grid.total - 1)]
            parts = [("ENV", (idx < b1) & own), ("ORCA", (idx >= b1) & (idx < b2) & own),
                     ("ROWS", (idx >= b2) & (idx < b3) & own), ("STATE", (idx >= b3) & own)]
        else:
            parts = [(TAGS[tag], np.ones(len(idx), bool))]
        base_all = rows[:, 0].astype(np.int64).min()
        if tag == 2:
            launch0 = base_all
        for name, sel in parts:
            if sel.any():
                report(np, name, rows[sel], launch0 if tag == 3 and launch0 is not None else base_all)
        if tag == 2 and len(idx) == grid.total:
            # what each STATE wave waited for: the ORCA waves and the ENV waves of its envs
            end = (rows[:, 1].astype(np.int64) - base_all) / 100.0
            start = (rows[:, 0].astype(np.int64) - base_all) / 100.0
            lag, info = [], []
            for sb in range(state_blocks):
                e0, e1 = grid.span("STATE", sb)
                if e1 <= e0:
                    continue
                envs = np.arange(e0, e1)
                ready_orca = end[np.unique(grid.block_of(np, "ORCA", np.arange(e0 * batch.N, e1 * batch.N)))].max()
                ready_env = end[np.unique(grid.block_of(np, "ENV", envs))].max()
                ready = max(ready_orca, ready_env)
                lag.append(end[b3 + sb] - ready)
                info.append((end[b3 + sb], ready_orca, ready_env, start[b3 + sb]))
            if rows[:, 4].any() and (rows[:, 4] >> np.uint64(32)).any():
                # where the waves of an env ran: its ENV, ROWS and STATE wave and the ORCA waves of its N humans
                xcc = (rows[:, 4] >> np.uint64(32)).astype(np.int64) & 15
                envs = np.arange(E)
                who = [grid.block_of(np, r, envs) for r in ("ENV", "ROWS", "STATE")]
                who += [grid.block_of(np, "ORCA", envs * batch.N + i) for i in range(batch.N)]
                per_env = np.sort(xcc[np.stack(who, axis=1)], axis=1)
                distinct = 1 + (np.diff(per_env, axis=1) != 0).sum(axis=1)
                # the deal itself: how many blocks ran on the XCD most blocks of their index mod 8 ran on
                cls = np.arange(grid.total) % 8
                home = np.array([np.bincount(xcc[cls == c], minlength=16).argmax() for c in range(8)])
                print("XCC: %.1f%% of envs had all their waves on one XCD; distinct XCDs per env p50 / max %d / %d; "
                      "%.1f%% of blocks ran on the XCD of their index mod 8 (%s)" % (
                          100.0 * (distinct == 1).mean(), np.percentile(distinct, 50), distinct.max(),
                          100.0 * (xcc == home[cls]).mean(), " ".join(str(h) for h in home)))
            lag = np.array(lag)
            print("STATE end minus (its last ORCA wave's end, its last ENV wave's end): p10/p50/p90/max %.2f %.2f %.2f %.2f us" % (
                np.percentile(lag, 10), np.percentile(lag, 50), np.percentile(lag, 90), lag.max()))
            last = np.argsort([q[0] for q in info])[-6:]
            print("   the 6 STATE waves that ended last (end, last ORCA end, ENV end, own start): " +
                  " ".join("(%.1f %.1f %.1f %.1f)" % info[q] for q in last))


class StepGrid:
    """csrc/ebc_step_grid.h, restated: eight classes of ec = ceil(E / 8) consecutive envs; block r of a role works for
    class r % 8, rank r // 8, on `upw` units (envs; ORCA: flat humans) of it; every role takes 8 Q blocks."""

    def __init__(self, E, N, hpw, rows_epw):
        self.E, self.N = E, N
        self.ec = -(-E // 8)
        self.upw = {"ENV": 16, "ORCA": hpw, "ROWS": rows_epw, "STATE": 64 // N}
        self.per_class = {r: self.ec * (N if r == "ORCA" else 1) for r in self.upw}
        self.units = {r: E * (N if r == "ORCA" else 1) for r in self.upw}
        self.blocks = {r: 8 * -(-self.per_class[r] // self.upw[r]) for r in self.upw}
        self.base, at = {}, 0
        for r in ("ENV", "ORCA", "ROWS", "STATE"):
            self.base[r] = at
            at += self.blocks[r]
        self.total = at

    def span(self, role, r):
        c, q = r % 8, r // 8
        lo = c * self.per_class[role]
        first = lo + q * self.upw[role]
        return first, min(first + self.upw[role], lo + self.per_class[role], self.units[role])

    def owns(self, np, role):
        return np.array([self.span(role, r)[1] > self.span(role, r)[0] for r in range(self.blocks[role])])

    def block_of(self, np, role, units):
        """the block (index in the launch) that owns these units"""
        c = units // self.per_class[role]
        return self.base[role] + (units - c * self.per_class[role]) // self.upw[role] * 8 + c


def head_segments(np, segments, stored, have):
    """The head of a consumer wave (marks build): each segment's length in us, p10 / p50 / p90 over the role's waves and
    for the six waves that stored last.  Only waves that passed every mark of the head (`have`) count: a mark inside a
    branch no lane took (STATE's restart scene without auto-reset, or in a wave without a live env) stays 0."""
    if not have.any():
        print("   head segments: no wave passed every mark of the head")
        return
    if not have.all():
        print("   head segments over the %d of %d waves that passed every mark of the head" % (have.sum(), len(have)))
    order = np.argsort(stored)
    last = order[have[order]][-6:]
    pct = lambda v: "%.2f / %.2f / %.2f" % tuple(np.percentile(v[have], (10, 50, 90)))
    print("   head segments, p10 / p50 / p90 us: " + ", ".join("%s %s" % (n, pct(v)) for n, v in segments))
    print("   head segments of the 6 that stored last: " + " ".join(
        "(" + " ".join("%.2f" % v[q] for _, v in segments) + ")" for q in last))


def report(np, name, rows, base):
    r0, r1 = rows[:, 0].astype(np.int64), rows[:, 1].astype(np.int64)
    cyc = (rows[:, 3] - rows[:, 2]).astype(np.int64)
    us = lambda x: (x - base) / 100.0
    life = (r1 - r0) / 100.0
    mhz = np.median(cyc[life > 0] / life[life > 0])
    print("%s: %d waves; starts %.2f..%.2f us, last end %.2f us" % (
        name, len(rows), us(r0.min()), us(r0.max()), us(r1.max())))
    print("   lifetime us p10/p50/p90/max: %.2f %.2f %.2f %.2f; shader clock ~%.0f MHz" % (
        np.percentile(life, 10), np.percentile(life, 50), np.percentile(life, 90), life.max(), mhz))
    edges = np.arange(0, us(r1.max()) + 1.0, 1.0)
    print("   resident waves at t = 0, 1, 2 ... us: " + " ".join(str(int(((us(r0) <= x) & (us(r1) > x)).sum())) for x in edges))
    print("   started by t:                        " + " ".join(str(int((us(r0) <= x).sum())) for x in edges))
    if name == "ENV" and rows[:, 6].any():  # marks 1 (action), 2 (quarters combined), 3 (grid), 4 (end)
        c0 = rows[:, 2].astype(np.int64)
        mk = rows[:, 6:10].astype(np.int64) - c0[:, None]
        names = ["start->robot action done", "publish + humans + distances + combine", "grid window", "reward + outputs"]
        segs = [mk[:, 0]] + [mk[:, q + 1] - mk[:, q] for q in range(3)]
        print("   cycles mean: " + ", ".join("%s %.0f" % (n, v.mean()) for n, v in zip(names, segs)))
        act = mk[:, 0] / (cyc / np.maximum(life, 1e-9))
        print("   start->robot action done, p10 / p50 / p90 us: %.2f / %.2f / %.2f" % tuple(np.percentile(act, (10, 50, 90))))
    if name == "ORCA":
        last = np.argsort(r1)[-8:]
        print("   the 8 waves that ended last (start us, lifetime us): " + " ".join("(%.1f, %.1f)" % (us(r0[q]), life[q]) for q in last))
    if name == "STATE" and rows[:, 5].any():
        c0 = rows[:, 2].astype(np.int64)
        mk = rows[:, 5:9].astype(np.int64)
        mhz = cyc / np.maximum(life, 1e-9)  # this wave's shader clock
        at = lambda q: us(r0) + (mk[:, q] - c0) / mhz  # a mark as us on the launch's time axis
        ready, woke, done_ = at(0), at(1), at(2)
        pct = lambda v: "%.1f / %.1f / %.1f" % (np.percentile(v, 10), np.percentile(v, 50), np.percentile(v, 90))
        print("   on the launch's time axis, p10 / p50 / p90 us: own loads ready %s, mailboxes all full %s, state stored %s" % (
            pct(ready), pct(woke), pct(done_)))
        print("   mailboxes full -> stored: %s us" % pct(done_ - woke))
        last = np.argsort(done_)[-6:]
        print("   the 6 that stored last (start, loads ready, mailboxes full, stored): " + " ".join(
            "(%.1f %.1f %.1f %.1f)" % (us(r0[q]), ready[q], woke[q], done_[q]) for q in last))
        if rows[:, 8].any():
            # the head, which the marks build waits for part by part (csrc/ebc_kernels.h, state_role): marks 3 (arguments
            # staged), 4 (state batch back), 5 (restart scene and pool.pref back), 0 (restart robot copied into LDS)
            mk = rows[:, 5:11].astype(np.int64)
            head_segments(np, [("start -> arguments staged", at(3) - us(r0)), ("-> state batch back", at(4) - at(3)),
                               ("-> restart scene back", at(5) - at(4)), ("-> restart robot parked", at(0) - at(5))],
                          done_, (mk[:, [0, 3, 4, 5]] != 0).all(axis=1))
    if name == "ROWS" and rows[:, 7].any():  # marks 0 (rows_loaded put), 1 (velocities in), 2 (rows stored)
        c0 = rows[:, 2].astype(np.int64)
        mk = rows[:, 5:11].astype(np.int64)
        mhz = cyc / np.maximum(life, 1e-9)
        at = lambda q: us(r0) + (mk[:, q] - c0) / mhz
        put, vel, stored = at(0), at(1), at(2)
        pct = lambda v: "%.1f / %.1f / %.1f" % (np.percentile(v, 10), np.percentile(v, 50), np.percentile(v, 90))
        print("   on the launch's time axis, p10 / p50 / p90 us: rows_loaded put %s, velocities in %s, rows stored %s" % (
            pct(put), pct(vel), pct(stored)))
        print("   velocities in -> rows stored: %s us; last rows stored %.1f us" % (pct(stored - vel), stored.max()))
        if rows[:, 8].any():  # the head: marks 3 (arguments staged), 4 (state back), 5 (robot_ready seen), 0 (robot_n back)
            head_segments(np, [("start -> arguments staged", at(3) - us(r0)), ("-> state back", at(4) - at(3)),
                               ("-> robot_ready seen", at(5) - at(4)), ("-> robot_n back", put - at(5))],
                          stored, (mk[:, [0, 3, 4, 5]] != 0).all(axis=1))
    if name == "ORCA" and rows[:, 5].any():
        c0 = rows[:, 2].astype(np.int64)
        marks = rows[:, 5:10].astype(np.int64) - c0[:, None]
        total = cyc
        names = ["loads", "rank", "lines", "LP2", "LP3", "end"]
        seg = np.concatenate([marks[:, :1], np.diff(marks, axis=1), (total - marks[:, 4])[:, None]], axis=1)
        lp1, lp3, lp3it = (rows[:, 11 + q].astype(np.int64) for q in range(3))
        order = np.argsort(life)
        for label, pick in (("median waves", order[len(order) // 2 - 50:len(order) // 2 + 50]),
                            ("slowest 1%", order[-max(1, len(order) // 100):])):
            print("   %s: cycles per segment " % label + ", ".join(
                "%s %.0f" % (n, seg[pick, q].mean()) for q, n in enumerate(names)) +
                "; LP1 calls %.1f, LP3 entered %.2f, LP3 rounds %.1f" % (lp1[pick].mean(), lp3[pick].mean(), lp3it[pick].mean()))
        prev = rows[:, 15].astype(np.int64)
        both = ((lp3 > 0) & (prev > 0)).sum()
        print("   waves entering LP3 this launch %d, the launch before %d, both %d (of %d waves)" % ((lp3 > 0).sum(), (prev > 0).sum(), both, len(lp3)))
        print("   LP1 calls per wave: mean %.2f p50 %d p90 %d max %d; waves entering LP3: %.1f%%" % (
            lp1.mean(), np.percentile(lp1, 50), np.percentile(lp1, 90), lp1.max(), 100.0 * (lp3 > 0).mean()))


if __name__ == "__main__":
    main()
