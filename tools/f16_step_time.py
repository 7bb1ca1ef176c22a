"""Step time of the north-star layer with float16 activation I/O (DAU_FLAG_IO_F16) against float32 I/O, same process, same
device, interleaved: N=128 C=256->256 56x56, G=4, max_kernel_size 9, mu ~ U(-3,3), sigma 0.5, forward + backward (dx, dw,
dmu1, dmu2, dsigma) through the plan API, as bench.py's plain step.  bench.py has no f16 option (and is not to be changed).

Each round times `--steps` back-to-back steps of one format with HIP events after `--warmup` untimed ones; the rounds
alternate fp32 / f16.  Prints one JSON line: per format the median and all per-step milliseconds (event time / steps of
each round), and the f16 / fp32 ratio of the medians.
usage: python tools/f16_step_time.py [--steps 20] [--warmup 5] [--rounds 4] [--only fp32|f16]"""
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
    ap.add_argument("--only", choices=("fp32", "f16"), default=None, help="one format only (e.g. under rocprofv3)")
    args = ap.parse_args()
    import torch
    from dau_conv import _capi

    N, S, F, H, W, G, k, m = 128, 256, 256, 56, 56, 4, 9, 3.0
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
    runs = {}
    for name, flag, dt in (("fp32", 0, torch.float32), ("f16", _capi.FLAG_IO_F16, torch.float16)):
        if args.only and name != args.only:
            continue
        plan = _capi.Plan(N, S, F, G, H, W, max_kernel_size=k, flags=_capi.FLAG_USE_INTERPOLATION | flag, sigma_hint=0.5,
                          mu_learning_rate_factor=1.0)
        runs[name] = (plan, x.to(dt), dy.to(dt))
    infos = {n: r[0].info for n, r in runs.items()}

    def step(plan, xi, dyi):
        plan.forward(xi, w, mu1, mu2, sigma)
        plan.backward(xi, dyi, w, mu1, mu2, sigma)

    times = {n: [] for n in runs}
    for _ in range(args.rounds):
        for name, (plan, xi, dyi) in runs.items():
            for _ in range(args.warmup):
                step(plan, xi, dyi)
            torch.cuda.synchronize()
            for _ in range(args.steps):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                step(plan, xi, dyi)
                b.record()
                times[name].append((a, b))
            torch.cuda.synchronize()
            plan.check_status()
    ms = {n: [round(a.elapsed_time(b), 4) for a, b in t] for n, t in times.items()}
    out = {"workload": "ns N=128 C=256->256 HW=56 G=4 k=9 mu~U(-3,3) fwd+bwd", "device": torch.cuda.get_device_name(0),
           "build_id": _capi.build_id(), "steps_per_round": args.steps, "rounds": args.rounds,
           "median_ms": {n: round(statistics.median(v), 4) for n, v in ms.items()}, "ms": ms,
           "plans_equal": len(infos) < 2 or infos["fp32"] == infos["f16"]}
    if len(ms) == 2:
        out["f16_over_fp32"] = round(out["median_ms"]["f16"] / out["median_ms"]["fp32"], 4)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
