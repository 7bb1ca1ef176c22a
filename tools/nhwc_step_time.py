"""Step time of the north-star layer on channels_last activations: the NHWC plan (DAU_FLAG_IO_NHWC) against converting around
the NCHW plan, same process, same device, interleaved: N=128 C=256->256 56x56, G=4, max_kernel_size 9, mu ~ U(-3,3), sigma 0.5,
forward + backward (dx, dw, dmu1, dmu2, dsigma) through the plan API, as bench.py's plain step (bench.py is not to be changed).

Three legs per storage format:
  nchw     the NCHW plan on contiguous tensors (the yardstick: what the layer costs without any layout work)
  convert  what a channels_last model pays around the NCHW plan: x.contiguous() once per step, y -> channels_last,
           dy.contiguous(), dx -> channels_last
  nhwc     the NHWC plan on the channels_last tensors
Each round times `--steps` back-to-back steps of one leg with HIP events after `--warmup` untimed ones; the rounds alternate the
legs.  Prints one JSON line: per format and leg the median over all steps, the median of every round (their spread is the noise
of the box), and nhwc - convert.
usage: python tools/nhwc_step_time.py [--steps 20] [--warmup 5] [--rounds 4] [--formats fp32,f16,bf16] [--only LEG]"""
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
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--formats", default="fp32,f16")
    ap.add_argument("--only", choices=("nchw", "convert", "nhwc"), default=None, help="one leg only (e.g. under rocprofv3)")
    args = ap.parse_args()
    import torch
    from dau_conv import _capi

    N, S, F, H, W, G, k, m = 128, 256, 256, 56, 56, 4, 9, 3.0
    CL = torch.channels_last
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev)
    gen.manual_seed(1234)
    x = torch.rand((N, S, H, W), device=dev, generator=gen)
    dy = torch.randn((N, F, H, W), device=dev, generator=gen)
    w = torch.randn((1, S, G, F), device=dev, generator=gen) * 0.1
    lim = k // 2 - 0.01
    mu1 = ((torch.rand((1, S, G, F), device=dev, generator=gen) * 2 - 1) * m).clamp_(-lim, lim)
    mu2 = ((torch.rand((1, S, G, F), device=dev, generator=gen) * 2 - 1) * m).clamp_(-lim, lim)
    sigma = torch.full((1, S, G, F), 0.5, device=dev)
    formats = {"fp32": (0, torch.float32), "f16": (_capi.FLAG_IO_F16, torch.float16), "bf16": (_capi.FLAG_IO_BF16, torch.bfloat16)}

    def make_plan(flags):
        return _capi.Plan(N, S, F, G, H, W, max_kernel_size=k, flags=_capi.FLAG_USE_INTERPOLATION | flags, sigma_hint=0.5,
                          mu_learning_rate_factor=1.0)

    def step_plain(plan, xi, dyi):
        plan.forward(xi, w, mu1, mu2, sigma)
        plan.backward(xi, dyi, w, mu1, mu2, sigma)

    def step_convert(plan, xi, dyi):
        xc = xi.contiguous()                                              # saved for backward, as the layer does
        plan.forward(xc, w, mu1, mu2, sigma).contiguous(memory_format=CL)
        plan.backward(xc, dyi.contiguous(), w, mu1, mu2, sigma)[0].contiguous(memory_format=CL)

    out = {"workload": "ns N=128 C=256->256 HW=56 G=4 k=9 mu~U(-3,3) fwd+bwd", "device": torch.cuda.get_device_name(0),
           "build_id": _capi.build_id(), "steps_per_round": args.steps, "rounds": args.rounds, "formats": {}}
    for fmt in args.formats.split(","):
        flag, dt = formats[fmt]
        nchw, nhwc = make_plan(flag), make_plan(flag | _capi.FLAG_IO_NHWC)
        xi, dyi = x.to(dt), dy.to(dt)
        xl, dyl = xi.contiguous(memory_format=CL), dyi.contiguous(memory_format=CL)
        legs = {"nchw": (step_plain, nchw, xi, dyi), "convert": (step_convert, nchw, xl, dyl), "nhwc": (step_plain, nhwc, xl, dyl)}
        if args.only:
            legs = {args.only: legs[args.only]}
        times = {n: [] for n in legs}
        for _ in range(args.rounds):
            for name, (fn, plan, a_x, a_dy) in legs.items():
                for _ in range(args.warmup):
                    fn(plan, a_x, a_dy)
                torch.cuda.synchronize()
                evs = []
                for _ in range(args.steps):
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    fn(plan, a_x, a_dy)
                    b.record()
                    evs.append((a, b))
                torch.cuda.synchronize()
                plan.check_status()
                times[name].append([a.elapsed_time(b) for a, b in evs])
        res = {"plans_equal": nchw.info == nhwc.info,
               "median_ms": {n: round(statistics.median([v for r in t for v in r]), 4) for n, t in times.items()},
               "round_median_ms": {n: [round(statistics.median(r), 4) for r in t] for n, t in times.items()}}
        if not args.only:
            res["nhwc_minus_convert_ms"] = round(res["median_ms"]["nhwc"] - res["median_ms"]["convert"], 4)
            res["convert_minus_nchw_ms"] = round(res["median_ms"]["convert"] - res["median_ms"]["nchw"], 4)
            res["nhwc_minus_nchw_ms"] = round(res["median_ms"]["nhwc"] - res["median_ms"]["nchw"], 4)
        out["formats"][fmt] = res
        del nchw, nhwc, xi, dyi, xl, dyl, legs
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
