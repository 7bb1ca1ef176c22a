"""Step time of a DAU layer behind BatchNorm and ReLU at the north-star shape, with the ReLU fused into the layer's loads
(DAU_FLAG_INPUT_RELU) against the ReLU module in front of it: same process, same device, interleaved.
N=128 C=256->256 56x56, G=4, max_kernel_size 9, mu ~ U(-3,3), sigma 0.5, forward + backward through autograd (dx through the
BatchNorm, its affine gradients, dw, dmu1, dmu2, dbias).

Two legs per input dtype (float32, float16, bfloat16) and layout (contiguous, channels_last):
  composed  BatchNorm2d -> ReLU -> DAUConv2d: the ReLU's forward pass (one read, one write of N*S*H*W), its backward pass (two reads,
            one write) and its saved output
  fused     BatchNorm2d -> DAUConv2d(input_activation="relu"): the layer takes the BatchNorm output, clamps it where it loads it and
            masks dx by it in the store; autograd saves the BatchNorm output only
Each round times `--steps` back-to-back steps of one leg with HIP events after `--warmup` untimed ones; the rounds alternate the
legs.  Prints one JSON line per (dtype, layout): the median over all steps, the median of every round (their spread is the noise of
the box), fused - composed, and torch.cuda.max_memory_allocated of a step of either leg.
usage: python tools/input_relu_step_time.py [--steps 10] [--warmup 3] [--rounds 5] [--formats fp32,f16,bf16] [--layouts nchw,nhwc]
                                            [--out FILE (appended)]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "dau-convnet_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--formats", default="fp32,f16,bf16")
    ap.add_argument("--layouts", default="nchw,nhwc")
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--out", default=None, help="JSON-lines file the result lines are appended to")
    args = ap.parse_args()
    import torch
    import torch.nn as nn
    import dau_conv
    from dau_conv import _capi

    N, S, F, H, W = args.batch, 256, 256, 56, 56
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev)
    gen.manual_seed(1234)
    x32 = torch.randn((N, S, H, W), device=dev, generator=gen)
    dtypes = {"fp32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}

    def make(fused, dt):
        torch.manual_seed(0)
        dau = dau_conv.DAUConv2d(filters=F, dau_units=(2, 2), max_kernel_size=9, in_channels=S, use_bias=True,
                                 mu1_initializer=dau_conv.random_uniform_initializer(-3, 3),
                                 mu2_initializer=dau_conv.random_uniform_initializer(-3, 3),
                                 bias_initializer=dau_conv.random_normal_initializer(stddev=0.5),
                                 mu_learning_rate_factor=1.0, input_activation="relu" if fused else None)
        mods = [nn.BatchNorm2d(S).to(dt)] + ([] if fused else [nn.ReLU()]) + [dau]
        return nn.Sequential(*mods).to(dev)

    def measure(nets, x, dy):
        def step(name):
            for p in nets[name].parameters():
                p.grad = None
            x.grad = None
            nets[name](x).backward(dy)

        times = {n: [] for n in nets}
        peak = {}
        for rnd in range(args.rounds):
            for name in nets:
                for _ in range(args.warmup):
                    step(name)
                torch.cuda.synchronize()
                if rnd == 0:
                    torch.cuda.reset_peak_memory_stats()
                evs = []
                for _ in range(args.steps):
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    step(name)
                    b.record()
                    evs.append((a, b))
                torch.cuda.synchronize()
                if rnd == 0:
                    peak[name] = int(torch.cuda.max_memory_allocated())
                dau_conv.check_pending_offsets()
                times[name].append([a.elapsed_time(b) for a, b in evs])
        res = {"median_ms": {n: round(statistics.median([v for r_ in t for v in r_]), 4) for n, t in times.items()},
               "round_median_ms": {n: [round(statistics.median(r_), 4) for r_ in t] for n, t in times.items()}}
        res["spread_ms"] = {n: round(max(r_) - min(r_), 4) for n, r_ in res["round_median_ms"].items()}
        res["fused_minus_composed_ms"] = round(res["median_ms"]["fused"] - res["median_ms"]["composed"], 4)
        res["max_memory_allocated_bytes"] = peak
        res["fused_minus_composed_bytes"] = peak["fused"] - peak["composed"]
        return res

    head = {"call": "input_relu_step_time",
            "workload": "ns N=%d C=256->256 HW=56 G=4 k=9 mu~U(-3,3) BatchNorm2d -> ReLU -> DAUConv2d fwd+bwd" % N,
            "device": torch.cuda.get_device_name(0), "build_id": _capi.build_id(), "steps_per_round": args.steps, "rounds": args.rounds}
    for fmt in [f for f in args.formats.split(",") if f]:
        dt = dtypes[fmt]
        for layout in [l for l in args.layouts.split(",") if l]:
            mf = torch.channels_last if layout == "nhwc" else torch.contiguous_format
            nets = {"composed": make(False, dt), "fused": make(True, dt)}
            x = x32.to(dt).contiguous(memory_format=mf).requires_grad_(True)
            with torch.no_grad():
                y = nets["composed"](x)
                same = bool(torch.equal(y, nets["fused"](x)))
            dy = torch.randn(y.shape, device=dev, generator=gen).to(dt).contiguous(memory_format=mf)
            del y
            line = json.dumps(dict(head, format=fmt, layout=layout, outputs_identical=same, **measure(nets, x, dy)))
            print(line, flush=True)
            if args.out:
                with open(args.out, "a") as f:
                    f.write(line + "\n")
            del x, dy, nets
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
