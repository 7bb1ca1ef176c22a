"""Step time of a DAUConv2d(use_bias=True, activation=torch.relu) layer at the north-star shape with its bias and ReLU fused into
the kernels' store (fused_epilogue=True) against the default layer, which adds the bias and applies the ReLU in torch: same
process, same device, interleaved.  N=128 C=256->256 56x56, G=4, max_kernel_size 9, mu ~ U(-3,3), sigma 0.5, forward + backward
through autograd (dx, dw, dmu1, dmu2, dbias).

Two legs per input dtype (float32; float16 and bfloat16 input, as an autocast stack hands it to the layer):
  unfused  fused_epilogue=False: y + bias (a 16-bit y is promoted to float32), torch.relu, and autograd's passes for both
  fused    fused_epilogue=True: the output keeps the input's dtype; backward takes the ReLU mask and the bias gradient in one pass
and, with --stack, a two-layer stack on float16 input: the unfused first layer hands the second one float32 (it then loads, stores
and saves fp32), the fused one float16.
Each round times `--steps` back-to-back steps of one leg with HIP events after `--warmup` untimed ones; the rounds alternate the
legs.  Prints one JSON line per leg group: the median over all steps, the median of every round (their spread is the noise of the
box), and fused - unfused.
usage: python tools/fused_epilogue_step_time.py [--steps 10] [--warmup 3] [--rounds 5] [--formats fp32,f16,bf16] [--stack]"""
import argparse
import copy
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
    ap.add_argument("--stack", action="store_true", help="also the two-layer stack on float16 input")
    args = ap.parse_args()
    import torch
    import dau_conv
    from dau_conv import _capi

    N, S, F, H, W = 128, 256, 256, 56, 56
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev)
    gen.manual_seed(1234)
    x32 = torch.rand((N, S, H, W), device=dev, generator=gen)
    dtypes = {"fp32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}

    def make(fused):
        torch.manual_seed(0)
        return dau_conv.DAUConv2d(filters=F, dau_units=(2, 2), max_kernel_size=9, in_channels=S, use_bias=True, activation=torch.relu,
                                  mu1_initializer=dau_conv.random_uniform_initializer(-3, 3),
                                  mu2_initializer=dau_conv.random_uniform_initializer(-3, 3),
                                  bias_initializer=dau_conv.random_normal_initializer(stddev=0.5),
                                  mu_learning_rate_factor=1.0, fused_epilogue=fused).to(dev)

    def step(net, x, dy):
        for p in net.parameters():
            p.grad = None
        x.grad = None
        net(x).backward(dy)

    def measure(legs):
        """legs: {name: (net, x, dy)} -> median_ms, round_median_ms"""
        times = {n: [] for n in legs}
        for _ in range(args.rounds):
            for name, (net, x, dy) in legs.items():
                for _ in range(args.warmup):
                    step(net, x, dy)
                torch.cuda.synchronize()
                evs = []
                for _ in range(args.steps):
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    step(net, x, dy)
                    b.record()
                    evs.append((a, b))
                torch.cuda.synchronize()
                dau_conv.check_pending_offsets()
                times[name].append([a.elapsed_time(b) for a, b in evs])
        res = {"median_ms": {n: round(statistics.median([v for r in t for v in r]), 4) for n, t in times.items()},
               "round_median_ms": {n: [round(statistics.median(r), 4) for r in t] for n, t in times.items()}}
        res["spread_ms"] = {n: round(max(r) - min(r), 4) for n, r in res["round_median_ms"].items()}
        res["fused_minus_unfused_ms"] = round(res["median_ms"]["fused"] - res["median_ms"]["unfused"], 4)
        return res

    head = {"workload": "ns N=128 C=256->256 HW=56 G=4 k=9 mu~U(-3,3) DAUConv2d(use_bias, relu) fwd+bwd", "device": torch.cuda.get_device_name(0),
            "build_id": _capi.build_id(), "steps_per_round": args.steps, "rounds": args.rounds}
    for fmt in [f for f in args.formats.split(",") if f]:
        dt = dtypes[fmt]
        x = x32.to(dt).requires_grad_(True)
        legs = {}
        for name, fused in (("unfused", False), ("fused", True)):
            net = make(fused)
            with torch.no_grad():
                y = net(x)
            legs[name] = (net, x, torch.randn(y.shape, device=dev, generator=gen).to(y.dtype))
            out_dtype = str(y.dtype).replace("torch.", "")
            head.setdefault("output_dtype", {}).setdefault(fmt, {})[name] = out_dtype
            del y
        print(json.dumps(dict(head, leg="layer", format=fmt, **measure(legs))), flush=True)
        del legs, x
        torch.cuda.empty_cache()
    if args.stack:
        x = x32.half().requires_grad_(True)
        legs = {}
        for name, fused in (("unfused", False), ("fused", True)):
            first = make(fused)
            net = torch.nn.Sequential(first, copy.deepcopy(first))
            with torch.no_grad():
                y = net(x)
            legs[name] = (net, x, torch.randn(y.shape, device=dev, generator=gen).to(y.dtype))
            del y
        print(json.dumps(dict(head, leg="two-layer stack", format="f16", **measure(legs))), flush=True)


if __name__ == "__main__":
    main()
