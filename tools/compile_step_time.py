"""Step time of a residual block of two DAU layers with their neighbours, eager against torch.compile (Inductor): same process, same
device, interleaved.  The block at the north-star layer size (N=128 C=256 56x56, G=4, max_kernel_size 9, mu ~ U(-3,3), sigma 0.5):

    Conv2d(3x3) -> BatchNorm2d -> ReLU -> DAUConv2d -> BatchNorm2d -> ReLU -> DAUConv2d -> (+ shortcut)

forward + backward through autograd (dx, the convolution's and the BatchNorms' gradients, dw, dmu1, dmu2 of both DAU layers).  Under
torch.compile each DAU layer is one opaque op (torch.ops.dau_conv.conv) running the kernels the eager layer runs; what can differ is
the elementwise work between them -- BatchNorm, ReLU, the shortcut add -- which Inductor fuses and eager runs kernel by kernel.

Two legs per input dtype (float32, float16 under autocast, bfloat16 by .bfloat16()) and layout (contiguous, channels_last):
  eager     the block as it is
  compiled  torch.compile(block) with --backend (default inductor)
Each round times `--steps` back-to-back steps of one leg with HIP events after `--warmup` untimed ones; the rounds alternate the legs.
One JSON line per (dtype, layout): the median over all steps, the median of every round (their spread is the noise of the box),
compiled - eager, the graph count and graph breaks of the compiled leg, and the largest difference of the two legs' outputs.

Every (dtype, layout) runs in a process of its own under its own time limit (`timeout`), and the tool stops at the first that fails:
usage: python tools/compile_step_time.py [--steps 10] [--warmup 3] [--rounds 5] [--formats fp32,f16,bf16] [--layouts nchw,nhwc]
                                         [--backend inductor] [--limit 300] [--out FILE (appended)]"""
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


def one(args, fmt, layout):
    import torch
    import torch.nn as nn
    import torch._dynamo
    from torch._dynamo.testing import CompileCounterWithBackend
    from torch._dynamo.utils import counters
    import dau_conv
    from dau_conv import _capi

    N, C, H, W = args.batch, 256, 56, 56
    dev = torch.device("cuda:0")
    dt = {"fp32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}[fmt]
    mf = torch.channels_last if layout == "nhwc" else torch.contiguous_format

    class Block(nn.Module):
        def __init__(self):
            super().__init__()
            dau = lambda: dau_conv.DAUConv2d(filters=C, dau_units=(2, 2), max_kernel_size=9, in_channels=C, use_bias=False,
                                             mu1_initializer=dau_conv.random_uniform_initializer(-3, 3),
                                             mu2_initializer=dau_conv.random_uniform_initializer(-3, 3), mu_learning_rate_factor=1.0)
            self.conv, self.bn1, self.dau1 = nn.Conv2d(C, C, 3, padding=1, bias=False), nn.BatchNorm2d(C), dau()
            self.bn2, self.dau2 = nn.BatchNorm2d(C), dau()

        def forward(self, x):
            h = torch.relu(self.bn1(self.conv(x)))
            h = torch.relu(self.bn2(self.dau1(h)))
            return self.dau2(h) + x

    torch.manual_seed(0)
    block = Block().to(dev).to(memory_format=mf)
    if fmt == "bf16":
        block = block.bfloat16()
    autocast = torch.float16 if fmt == "f16" else None
    io = torch.float32 if fmt == "f16" else dt           # (autocast: the block takes float32 and casts at the convolution)
    gen = torch.Generator(device=dev)
    gen.manual_seed(1234)
    x = torch.randn((N, C, H, W), device=dev, generator=gen).to(io).contiguous(memory_format=mf).requires_grad_(True)
    dy = torch.randn((N, C, H, W), device=dev, generator=gen).to(io).contiguous(memory_format=mf)
    counters.clear()
    cnt = CompileCounterWithBackend(args.backend)
    legs = {"eager": block, "compiled": torch.compile(block, backend=cnt)}

    def step(name):
        for p in block.parameters():
            p.grad = None
        x.grad = None
        with torch.autocast("cuda", dtype=autocast, enabled=autocast is not None):
            y = legs[name](x)
        y.backward(dy.to(y.dtype))
        return y

    y0, y1 = step("eager").detach().float(), step("compiled").detach().float()       # (training mode: the batch's own statistics)
    diff, scale = float((y0 - y1).abs().max()), float(y0.abs().max())
    del y0, y1
    times = {n: [] for n in legs}
    for rnd in range(args.rounds):
        for name in legs:
            for _ in range(args.warmup):
                step(name)
            torch.cuda.synchronize()
            evs = []
            for _ in range(args.steps):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                step(name)
                b.record()
                evs.append((a, b))
            torch.cuda.synchronize()
            dau_conv.check_pending_offsets()
            times[name].append([a.elapsed_time(b) for a, b in evs])
    res = {"median_ms": {n: round(statistics.median([v for r_ in t for v in r_]), 4) for n, t in times.items()},
           "round_median_ms": {n: [round(statistics.median(r_), 4) for r_ in t] for n, t in times.items()}}
    res["spread_ms"] = {n: round(max(r_) - min(r_), 4) for n, r_ in res["round_median_ms"].items()}
    res["compiled_minus_eager_ms"] = round(res["median_ms"]["compiled"] - res["median_ms"]["eager"], 4)
    line = dict(call="compile_step_time",
                workload="ns N=%d C=256 HW=56 G=4 k=9 mu~U(-3,3) Conv2d3x3 -> BN -> ReLU -> DAU -> BN -> ReLU -> DAU + shortcut fwd+bwd" % N,
                device=torch.cuda.get_device_name(0), build_id=_capi.build_id(), torch=torch.__version__, backend=args.backend,
                steps_per_round=args.steps, rounds=args.rounds, format=fmt, layout=layout, graphs=cnt.frame_count,
                graph_breaks=sum(counters["graph_break"].values()), output_max_abs_diff=diff, output_max_abs=scale, **res)
    print(json.dumps(line), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--formats", default="fp32,f16,bf16")
    ap.add_argument("--layouts", default="nchw,nhwc")
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--backend", default="inductor")
    ap.add_argument("--limit", type=int, default=300, help="seconds each (dtype, layout) process may take")
    ap.add_argument("--out", default=None, help="JSON-lines file the result lines are appended to")
    ap.add_argument("--one", default=None, metavar="FORMAT,LAYOUT", help="(internal) measure this one and print its line")
    args = ap.parse_args()
    if args.one:
        return one(args, *args.one.split(","))
    for fmt in [f for f in args.formats.split(",") if f]:
        for layout in [l for l in args.layouts.split(",") if l]:
            cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--one", "%s,%s" % (fmt, layout),
                   "--steps", str(args.steps), "--warmup", str(args.warmup), "--rounds", str(args.rounds), "--batch", str(args.batch),
                   "--backend", args.backend]
            done = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
            lines = [l for l in done.stdout.splitlines() if l.startswith("{")]
            if done.returncode != 0 or not lines:
                # a failed, killed or timed-out step ends the run: nothing more is started on the device
                print("compile_step_time: %s %s ended with status %d; stopping" % (fmt, layout, done.returncode), file=sys.stderr)
                sys.stdout.write(done.stdout)
                return done.returncode or 1
            print(lines[-1], flush=True)
            if args.out:
                with open(args.out, "a") as f:
                    f.write(lines[-1] + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
