"""Step time of the last layer of a residual block at the north-star shape, y = relu((dau(x) + bias) + shortcut), with the shortcut
added inside the kernels' store against the composition around the fused bias: same process, same device, interleaved.
N=128 C=256->256 56x56, G=4, max_kernel_size 9, mu ~ U(-3,3), sigma 0.5, forward + backward through autograd (dx, dshortcut, dw,
dmu1, dmu2, dbias).

Two legs per input dtype (float32; float16 and bfloat16 input and shortcut, as an autocast stack hands them to the layer):
  composed  DAUConv2d(fused_epilogue=True, activation=None): the bias in the store, then torch.relu(out + shortcut) -- two
            whole-tensor passes forward, an activation-sized temporary, autograd's passes for both backward
  fused     DAUConv2d(fused_epilogue=True, activation=torch.relu)(x, residual=shortcut): one store; backward takes the ReLU mask and
            the bias gradient in one pass and hands the same dz to the shortcut
Each round times `--steps` back-to-back steps of one leg with HIP events after `--warmup` untimed ones; the rounds alternate the
legs.  Prints one JSON line per dtype: the median over all steps, the median of every round (their spread is the noise of the box),
and fused - composed.
usage: python tools/residual_step_time.py [--steps 10] [--warmup 3] [--rounds 5] [--formats fp32,f16,bf16] [--out FILE (appended)]"""
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
    ap.add_argument("--out", default=None, help="JSON-lines file the result lines are appended to")
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

    def make(activation):
        torch.manual_seed(0)
        return dau_conv.DAUConv2d(filters=F, dau_units=(2, 2), max_kernel_size=9, in_channels=S, use_bias=True, activation=activation,
                                  mu1_initializer=dau_conv.random_uniform_initializer(-3, 3),
                                  mu2_initializer=dau_conv.random_uniform_initializer(-3, 3),
                                  bias_initializer=dau_conv.random_normal_initializer(stddev=0.5),
                                  mu_learning_rate_factor=1.0, fused_epilogue=True).to(dev)

    composed_net, fused_net = make(None), make(torch.relu)
    forwards = {"composed": lambda x, r: torch.relu(composed_net(x) + r), "fused": lambda x, r: fused_net(x, residual=r)}
    nets = {"composed": composed_net, "fused": fused_net}

    def step(name, x, r, dy):
        for p in nets[name].parameters():
            p.grad = None
        x.grad = None
        r.grad = None
        forwards[name](x, r).backward(dy)

    def measure(x, r, dy):
        times = {n: [] for n in forwards}
        for _ in range(args.rounds):
            for name in forwards:
                for _ in range(args.warmup):
                    step(name, x, r, dy)
                torch.cuda.synchronize()
                evs = []
                for _ in range(args.steps):
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    step(name, x, r, dy)
                    b.record()
                    evs.append((a, b))
                torch.cuda.synchronize()
                dau_conv.check_pending_offsets()
                times[name].append([a.elapsed_time(b) for a, b in evs])
        res = {"median_ms": {n: round(statistics.median([v for r_ in t for v in r_]), 4) for n, t in times.items()},
               "round_median_ms": {n: [round(statistics.median(r_), 4) for r_ in t] for n, t in times.items()}}
        res["spread_ms"] = {n: round(max(r_) - min(r_), 4) for n, r_ in res["round_median_ms"].items()}
        res["fused_minus_composed_ms"] = round(res["median_ms"]["fused"] - res["median_ms"]["composed"], 4)
        return res

    head = {"call": "residual_step_time", "workload": "ns N=128 C=256->256 HW=56 G=4 k=9 mu~U(-3,3) relu((dau(x) + bias) + shortcut) fwd+bwd",
            "device": torch.cuda.get_device_name(0), "build_id": _capi.build_id(), "steps_per_round": args.steps, "rounds": args.rounds}
    for fmt in [f for f in args.formats.split(",") if f]:
        dt = dtypes[fmt]
        x = x32.to(dt).requires_grad_(True)
        with torch.no_grad():
            y = composed_net(x)
            # the shortcut at the size of the branch, so that the ReLU cuts about half
            r = (torch.randn(y.shape, device=dev, generator=gen) * y.float().std()).to(dt)
            same = bool(torch.equal(torch.relu(y + r), fused_net(x, residual=r))) if fmt == "fp32" else None
            out_dtype = {n: str(f(x, r).dtype).replace("torch.", "") for n, f in forwards.items()}
        r.requires_grad_(True)
        dy = torch.randn(y.shape, device=dev, generator=gen).to(dt)
        del y
        line = json.dumps(dict(head, format=fmt, output_dtype=out_dtype, fp32_outputs_identical=same, **measure(x, r, dy)))
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")
        del x, r, dy
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
