#!/usr/bin/env python3
"""Deciding with the wide SARL networks on the device: SarlValueNet(..., wide=True) (the wide two-layer blocks of
csrc/ebc_vn_wide.h, refinement included) against wide=False (torch's float32 GEMMs: what such a network decided on before)
in the same run, alternating, on the same rows; then every wide block of the x4 network alone.

    python3 tools/vn_wide_bench.py [--envs 1024] [--rows 5,18,30] [--repeats 7] [--out profiles/vn_wide.txt]
    python3 tools/vn_wide_bench.py --resource-usage      (no GPU: the compiler's registers / LDS / scratch per kernel)

Workload: a decision batch of `--envs` envs x 81 actions at R rows per state, random rows, random-init weights
(torch's Linear initialisation), for the x3 and x4 networks and, as the control, the x2 agent-type network, whose blocks
are narrow either way.  Chunks as DeviceSarlPolicy cuts them (2^21 rows).  Times: device events around one
action_values call, `--repeats` calls per form after two warm-up calls, the forms alternating; median and min .. max.
The blocks alone: microseconds per forward (both layers) and the share of the bf16 matrix peak (2.5 PFLOP/s dense) of
the 3 bf16 products per float32 product over the padded tiles the kernel multiplies; the float32 form on fewer rows (it
is the form of the few re-evaluated candidates) against the float32 matrix peak (157.3 TFLOP/s)."""
import argparse
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "eb-cadrl_amd")):
    sys.path.insert(0, p)

NETWORKS = (("x3", dict(mlp1=(400, 300), mlp2=(300, 100), attention=(300, 300, 1), mlp3=(400, 300, 300, 1))),
            ("x4", dict(mlp1=(600, 400), mlp2=(400, 200), attention=(400, 400, 1), mlp3=(600, 400, 400, 1))),
            ("x2 (control: narrow blocks either way)", dict(mlp1=(300, 200), mlp2=(200, 100), attention=(200, 200, 1), mlp3=(300, 200, 200, 1))))
T, ACTIONS, SELF = 17, 81, 6
BF16_PEAK, F32_PEAK = 2.5e15, 157.3e12


def state_dict(dims, seed):
    import torch
    torch.manual_seed(seed)
    sd = {}

    def stack(prefix, fan_in, widths):
        for i, o in enumerate(widths):
            lin = torch.nn.Linear(fan_in, o)
            sd["%s.%d.weight" % (prefix, 2 * i)], sd["%s.%d.bias" % (prefix, 2 * i)] = lin.weight.detach(), lin.bias.detach()
            fan_in = o
    stack("mlp1", T, dims["mlp1"])
    stack("mlp2", dims["mlp1"][-1], dims["mlp2"])
    stack("attention", 2 * dims["mlp1"][-1], dims["attention"])
    stack("mlp3", SELF + dims["mlp2"][-1], dims["mlp3"])
    return sd


def timed(fn, repeats):
    """-> milliseconds per call of every fn of `fn` (a dict), the calls alternating between them."""
    import torch
    for _ in range(2):
        for f in fn.values():
            f()
    torch.cuda.synchronize()
    ms = {k: [] for k in fn}
    for _ in range(repeats):
        for k, f in fn.items():
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            ev[0].record()
            f()
            ev[1].record()
            torch.cuda.synchronize()
            ms[k].append(ev[0].elapsed_time(ev[1]))
    return ms


def spread(v):
    return "%.2f ms (%.2f .. %.2f)" % (statistics.median(v), min(v), max(v))


def clocks():
    try:
        out = subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=60).stdout
        keep = [line.strip() for line in out.splitlines() if "GPU[0]" in line and ("sclk" in line or "mclk" in line)]
        return "; ".join(keep) or "not read"
    except Exception:
        return "not read"


def resource_usage():
    """The new unit compiled with -Rpass-analysis=kernel-resource-usage: one line per kernel."""
    csrc = os.path.join(ROOT, "eb-cadrl_amd", "csrc")
    cmd = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=off",
           "-fno-fast-math", "-fno-gpu-flush-denormals-to-zero", "-mllvm", "-amdgpu-kernarg-preload-count=14",
           "-Rpass-analysis=kernel-resource-usage", "-c", "-o", os.devnull, "ebcsim_vn_wide.hip"]
    err = subprocess.run(cmd, cwd=csrc, capture_output=True, text=True, check=True).stderr
    lines, cur = [], []
    for line in err.splitlines():
        if "remark:" not in line:
            continue
        text = line.split("remark:", 1)[1].replace("[-Rpass-analysis=kernel-resource-usage]", "").strip()
        if text.startswith("Function Name"):
            if cur:
                lines.append(", ".join(cur))
            cur = [text.split(":", 1)[1].strip()]
        elif text.split(":")[0] in ("VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "LDS Size [bytes/block]", "SGPRs"):
            cur.append(text)
    if cur:
        lines.append(", ".join(cur))
    return ["# hipcc -Rpass-analysis=kernel-resource-usage, ebcsim_vn_wide.hip (dynamic LDS is not in 'LDS Size': layer 1 takes 94208 B, layer 2 57344 B)"] + lines


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--envs", type=int, default=1024)
    ap.add_argument("--rows", default="5,18,30")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--block-rows", type=int, default=1024 * 81 * 18)
    ap.add_argument("--f32-rows", type=int, default=1 << 15)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vn_wide.txt"))
    ap.add_argument("--resource-usage", action="store_true", help="only the compiler's resource usage of the new kernels (no GPU)")
    args = ap.parse_args()
    if args.resource_usage:
        print("\n".join(resource_usage()))
        return
    import torch
    from ebcsim.mlp2 import Mlp2Block
    from ebcsim.sarl import SarlValueNet
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    dev = torch.device("cuda", 0)
    out = ["# python3 tools/vn_wide_bench.py --envs %d --rows %s --repeats %d" % (args.envs, args.rows, args.repeats),
           "# %s; clocks: %s" % (torch.cuda.get_device_name(0), clocks()),
           "# one action_values call (sweep of envs x 81 actions x R rows + refinement), device events, median (min .. max) of %d, forms alternating" % args.repeats]
    g = torch.Generator().manual_seed(1)
    for name, dims in NETWORKS:
        sd = state_dict(dims, 7)
        nets = {w: SarlValueNet(sd, device="cuda:0", wide=w) for w in (True, False)}
        for R in (int(r) for r in args.rows.split(",")):
            rows = torch.randn(args.envs, ACTIONS, R, T, generator=g).to(dev)
            reward = (torch.rand(args.envs, ACTIONS, generator=g).double() * 0.01).to(dev)
            chunk = max(1, (1 << 21) // R)
            fn = {w: (lambda n=n: n.action_values(rows, reward, 0.9, chunk_pairs=chunk)) for w, n in nets.items()}
            before = nets[True].refine_stats or {}
            ms = timed(fn, args.repeats)
            a, b = statistics.median(ms[True]), statistics.median(ms[False])
            with torch.no_grad():
                paths = {w: n.path_for(rows.reshape(-1, R, T)[:1]) for w, n in nets.items()}
            st = {k: v - before.get(k, 0) for k, v in (nets[True].refine_stats or {}).items()}  # of this R's calls
            per = st.get("candidates", 0) / max(1, st.get("decisions", 1))
            verdict = "%.2fx faster" % (b / a) if a < b else "SLOWER, %.2fx" % (a / b)
            out.append("%s R %d: wide=True [%s] %s | wide=False [%s] %s | wide is %s; candidates per decision %.2f, coarse_eps %s, bound violations %d" % (
                name, R, paths[True], spread(ms[True]), paths[False], spread(ms[False]), verdict, per,
                "%.3g" % nets[True].coarse_eps if nets[True].coarse_eps else "-", st.get("bound_violations", 0)))
            print(out[-1], flush=True)
            del rows
        del nets
        torch.cuda.empty_cache()
    # ---- the wide blocks of the x4 network alone
    out.append("# the x4 network's blocks alone: coarse form on %d rows, float32 form on %d rows; us per forward (both layers), median (min .. max)" % (
        args.block_rows, args.f32_rows))
    tiles = lambda n: (n + 31) // 32 * 32  # noqa: E731
    for label, (K0, H, O), tail, group in (("mlp1", (T, 600, 400), False, 0), ("mlp2", (400, 400, 200), False, 0),
                                            ("attention", (400, 400, 400), True, 18), ("mlp3[:2]", (206, 600, 400), False, 0)):
        lin = lambda o, i: (torch.randn(o, i, generator=g) / i ** 0.5, torch.randn(o, generator=g) * 0.1)  # noqa: E731
        fin = (torch.randn(1, O, generator=g) / O ** 0.5, torch.randn(1, generator=g)) if tail else None
        blk = Mlp2Block([lin(H, K0), lin(O, H)], 0, final=fin, wide=True)
        for form, M, peak, per_mac in (("coarse", args.block_rows, BF16_PEAK, 3), ("float32", args.f32_rows, F32_PEAK, 1)):
            x = torch.randn(M, K0, generator=g).to(dev)
            rb = torch.randn(-(-M // group), H, generator=g).to(dev) if group else None
            y = torch.empty((M,) if tail else (M, O), dtype=torch.float32, device=dev)
            entry = blk if form == "coarse" else blk.f32
            ms = timed({0: lambda: entry(x, False, row_bias=rb, group_rows=group, out=y)}, args.repeats)[0]
            padded = (tiles(K0) if form == "coarse" else K0) * tiles(H) + tiles(H) * tiles(O)
            flops = 2.0 * per_mac * padded * M
            med = statistics.median(ms)
            out.append("%s %d x %d x %d%s %s: %.1f us (%.1f .. %.1f), %.1f TFLOP/s issued = %.1f %% of the %s matrix peak" % (
                label, K0, H, O, " + tail + group term" if tail else "", form, med * 1e3, min(ms) * 1e3, max(ms) * 1e3,
                flops / (med * 1e-3) / 1e12, 100.0 * flops / (med * 1e-3) / peak, "bf16" if form == "coarse" else "float32"))
            print(out[-1], flush=True)
            del x, y
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(out) + "\n")
    print("wrote %s" % args.out)


if __name__ == "__main__":
    main()
