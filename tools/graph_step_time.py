"""Step time of DAU layers run three ways: eager, as a replayed graph (torch.cuda.graph) and under
torch.compile(mode="reduce-overhead") (Inductor with its cudagraph trees) -- same process, same device, interleaved.  Forward +
backward through autograd (dx and every parameter gradient) at three sizes:

  harness  the reference's own speed harness (plugins/tensorflow/tests/dau_conv_test.py:504-628): one layer, N=32, 128 -> 32
           channels, 16 x 16, 2 units, max_kernel_size 9 -- a launch-bound step
  stack    three stacked DAUConv2d(96, (2, 2), 9, fused_epilogue=True) with ReLU on 128 x 96 x 32 x 32
  ns       the north-star layer, N=128, 256 -> 256 channels, 56 x 56, 2 x 2 units, max_kernel_size 9 -- a kernel-bound step

All three legs run the same kernels; what differs is what the host does per step: eager launches 25 to 45 kernels per layer and
pass from Python, most of them guarded kernels that return at once; a replay launches one graph.  Each round times `--steps`
back-to-back steps of one leg with HIP events after `--warmup` untimed ones; the rounds alternate the legs.  One JSON line per size:
the median over all steps, the median of every round (their spread is the noise of the box), the differences to eager, whether a
difference exceeds three times the larger round spread (only then is it a gain), the largest difference of the legs' outputs, and
per leg the peak of torch.cuda.max_memory_allocated above what was allocated before the leg was set up (eager: with the shared
workspace it creates; graph: what the capture allocated in its pool; compiled: warm-up, recording and first replays).

Every size runs in a process of its own under its own time limit (`timeout`), and the tool stops at the first that fails:
usage: python tools/graph_step_time.py [--steps 10] [--warmup 3] [--rounds 5] [--sizes harness,stack,ns] [--legs eager,graph,compiled]
                                       [--limit 400] [--out FILE (appended)]"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "dau-convnet_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

SIZES = {
    "harness": dict(N=32, S=128, F=32, H=16, W=16, units=(2, 1), layers=1, fused=False,
                    label="reference speed harness N=32 C=128->32 HW=16 G=2 k=9, one layer"),
    "stack": dict(N=128, S=96, F=96, H=32, W=32, units=(2, 2), layers=3, fused=True,
                  label="3 x DAUConv2d(96, (2,2), 9, fused_epilogue=True, relu) on 128x96x32x32"),
    "ns": dict(N=128, S=256, F=256, H=56, W=56, units=(2, 2), layers=1, fused=False,
               label="north-star layer N=128 C=256->256 HW=56 G=4 k=9"),
}


def one(args, size):
    import torch
    import torch.nn as nn
    import dau_conv
    from dau_conv import _capi

    cfg = SIZES[size]
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    init = dau_conv.random_uniform_initializer(-3, 3)
    layers, cin = [], cfg["S"]
    for _ in range(cfg["layers"]):
        layers.append(dau_conv.DAUConv2d(filters=cfg["F"], dau_units=cfg["units"], max_kernel_size=9, in_channels=cin,
                                         mu1_initializer=init, mu2_initializer=init, mu_learning_rate_factor=1.0,
                                         use_bias=cfg["fused"], fused_epilogue=cfg["fused"], activation=torch.relu if cfg["fused"] else None))
        cin = cfg["F"]
    model = nn.Sequential(*layers).to(dev)
    gen = torch.Generator(device=dev)
    gen.manual_seed(1234)
    x = torch.rand((cfg["N"], cfg["S"], cfg["H"], cfg["W"]), device=dev, generator=gen).requires_grad_(True)
    dy = torch.randn((cfg["N"], cfg["F"], cfg["H"], cfg["W"]), device=dev, generator=gen)
    names = [n for n in args.legs.split(",") if n]

    def step(fn):
        x.grad = None
        model.zero_grad(set_to_none=True)
        y = fn(x)
        y.backward(dy)
        return y

    legs, peak = {}, {}

    def setup(name):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        if name == "eager":
            legs[name] = lambda: step(model)
        elif name == "graph":
            step(model)                                      # every plan's first call is an ordinary one
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                static_y = step(model)

            def replay():
                graph.replay()
                return static_y
            legs[name] = replay
        else:
            compiled = torch.compile(model, mode="reduce-overhead")

            def run():
                torch.compiler.cudagraph_mark_step_begin()
                return step(compiled)
            legs[name] = run
        for _ in range(3):                                   # (the cudagraph trees warm up, record, replay)
            y = legs[name]()
        torch.cuda.synchronize()
        peak[name] = torch.cuda.max_memory_allocated() - base
        return y.detach().float().clone()

    ys = {n: setup(n) for n in names}
    scale = float(ys[names[0]].abs().max())
    diffs = {n: float((ys[n] - ys[names[0]]).abs().max()) for n in names[1:]}
    del ys
    times = {n: [] for n in names}
    for rnd in range(args.rounds):
        for name in names:
            for _ in range(args.warmup):
                legs[name]()
            torch.cuda.synchronize()
            evs = []
            for _ in range(args.steps):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                legs[name]()
                b.record()
                evs.append((a, b))
            torch.cuda.synchronize()
            times[name].append([a.elapsed_time(b) for a, b in evs])
    dau_conv.check_pending_offsets()
    res = {"median_ms": {n: round(statistics.median([v for r_ in t for v in r_]), 4) for n, t in times.items()},
           "round_median_ms": {n: [round(statistics.median(r_), 4) for r_ in t] for n, t in times.items()}}
    res["spread_ms"] = {n: round(max(r_) - min(r_), 4) for n, r_ in res["round_median_ms"].items()}
    noise = max(res["spread_ms"].values())
    res["minus_eager_ms"] = {n: round(res["median_ms"][n] - res["median_ms"]["eager"], 4) for n in names if n != "eager" and "eager" in names}
    res["gain_beyond_3_spreads"] = {n: bool(-d > 3 * noise) for n, d in res["minus_eager_ms"].items()}
    line = dict(call="graph_step_time", size=size, workload=cfg["label"] + " mu~U(-3,3) sigma=0.5 fp32 fwd+bwd",
                device=torch.cuda.get_device_name(0), build_id=_capi.build_id(), torch=torch.__version__,
                steps_per_round=args.steps, rounds=args.rounds, output_max_abs_diff_to_eager=diffs, output_max_abs=scale,
                peak_allocated_bytes_above_setup=peak, **res)
    print(json.dumps(line), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--sizes", default="harness,stack,ns")
    ap.add_argument("--legs", default="eager,graph,compiled")
    ap.add_argument("--limit", type=int, default=400, help="seconds each size's process may take")
    ap.add_argument("--out", default=None, help="JSON-lines file the result lines are appended to")
    ap.add_argument("--one", default=None, metavar="SIZE", help="(internal) measure this one and print its line")
    args = ap.parse_args()
    if args.one:
        return one(args, args.one)
    for size in [s for s in args.sizes.split(",") if s]:
        cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--one", size, "--steps", str(args.steps),
               "--warmup", str(args.warmup), "--rounds", str(args.rounds), "--legs", args.legs]
        done = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        lines = [l for l in done.stdout.splitlines() if l.startswith("{")]
        if done.returncode != 0 or not lines:
            # a failed, killed or timed-out step ends the run: nothing more is started on the device
            print("graph_step_time: %s ended with status %d; stopping" % (size, done.returncode), file=sys.stderr)
            sys.stdout.write(done.stdout)
            return done.returncode or 1
        print(lines[-1], flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(lines[-1] + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
