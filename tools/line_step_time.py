"""Step time of a single-dimension DAU layer (DAUConv1d) at the north-star size with the line members of the two-limb gather-sum
(dense_line=True, DAU_FLAG_DENSE_SPLIT_LINE) against the same layer without them: same process, same library, interleaved.
N=128 C=256->256 56x56, four units on the line, sigma 0.5, forward + backward through autograd (dx, dw, dmu1, dbias).

Two layers per input dtype (float32, bfloat16):
  k9   max_kernel_size 9,  mu1 ~ U(-3.99, 3.99): flag off = the 2-D two-limb members (9 x 9 taps), flag on = the 1 x 9 line member
  k17  max_kernel_size 17, mu1 ~ U(-7.99, 7.99): flag off = the exact gather of bucket 8,           flag on = the 1 x 17 line member
Each round times `--steps` back-to-back steps of one leg with HIP events after `--warmup` untimed ones; the rounds alternate the
legs.  Prints one JSON line per (layer, dtype): the median over all steps, the median of every round (their spread is the noise of
the box), on - off, the per-pass gather-sum times of dau_conv_profile_begin / _end (the dominant kernel of the pass: the GEMM or the
exact gather, without its staging) for either leg, which member the device took, and whether y agrees within the fp32 bar.
--line-grads: the line members of the two-limb gather-dot instead (dense_line_grads=True, DAU_FLAG_SPLIT_DOT_LINE).  Both legs then
have dense_line=True; flag off = the exact fp32 gather-dot of bucket 4 / 8, flag on = the line gather-dot of radius 4 / 8.  The
result lines also carry the per-pass gather-dot time of either leg and what dau_conv_dot_line_status reports.
usage: python tools/line_step_time.py [--steps 10] [--warmup 3] [--rounds 5] [--formats fp32,bf16] [--layers k9,k17] [--batch 128]
                                      [--line-grads] [--out FILE (appended)]"""
import argparse
import importlib
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "dau-convnet_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

LAYERS = {"k9": (9, 3.99), "k17": (17, 7.99)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--formats", default="fp32,bf16")
    ap.add_argument("--layers", default="k9,k17")
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--line-grads", action="store_true", help="time dense_line_grads=True against dense_line=True alone")
    ap.add_argument("--out", default=None, help="JSON-lines file the result lines are appended to")
    args = ap.parse_args()
    import torch
    import dau_conv
    from dau_conv import _capi
    dc = importlib.import_module("dau_conv.dau_conv")

    N, S, F, H, W = args.batch, 256, 256, 56, 56
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev)
    gen.manual_seed(1234)
    x32 = torch.rand((N, S, H, W), device=dev, generator=gen)
    dtypes = {"fp32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}

    def make(k, m, line):
        torch.manual_seed(0)
        return dau_conv.DAUConv1d(filters=F, dau_units=(4, 1), max_kernel_size=k, in_channels=S, use_bias=True,
                                  mu1_initializer=dau_conv.random_uniform_initializer(-m, m), mu_learning_rate_factor=1.0,
                                  dense_line=line or args.line_grads, dense_line_grads=line and args.line_grads).to(dev)

    def measure(nets, x, dy):
        def step(name):
            for p in nets[name].parameters():
                p.grad = None
            x.grad = None
            nets[name](x).backward(dy)

        times = {n: [] for n in nets}
        for rnd in range(args.rounds):
            for name in nets:
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
        res["on_minus_off_ms"] = round(res["median_ms"]["on"] - res["median_ms"]["off"], 4)
        # per-pass times of the gather-sum's dominant kernel, and the member the device took
        res["gather_sum_ms_per_pass"], res["line_status"] = {}, {}
        for name in nets:
            plan = nets[name]._line_plan
            plan.profile_begin()
            for _ in range(args.steps):
                step(name)
            torch.cuda.synchronize()
            prof = plan.profile_end()
            res["gather_sum_ms_per_pass"][name] = {k_: round(ms / max(n_, 1), 4) for k_, (ms, n_) in prof.items() if k_ != "gather_dot"}
            res["line_status"][name] = list(plan.line_status())
            if args.line_grads:
                ms, n_ = prof["gather_dot"]
                res.setdefault("gather_dot_ms_per_pass", {})[name] = round(ms / max(n_, 1), 4)
                res.setdefault("dot_line_status", {})[name] = list(plan.dot_line_status())
        return res

    head = {"call": "line_step_time_grads" if args.line_grads else "line_step_time", "device": torch.cuda.get_device_name(0), "build_id": _capi.build_id(),
            "steps_per_round": args.steps, "rounds": args.rounds}
    for layer in [l for l in args.layers.split(",") if l]:
        k, m = LAYERS[layer]
        for fmt in [f for f in args.formats.split(",") if f]:
            dt = dtypes[fmt]
            x = x32.to(dt).requires_grad_(True)
            nets, ys = {}, {}
            for name, line in (("off", False), ("on", True)):
                before = set(dc._PLANS)
                nets[name] = make(k, m, line)
                with torch.no_grad():
                    ys[name] = nets[name](x).float()
                (nets[name]._line_plan,) = [v for key, v in dc._PLANS.items() if key not in before]   # the plan this layer's calls run on
                nets[name]._line_info = nets[name]._line_plan.info["gather_dense_split"]
            err = float((ys["on"] - ys["off"]).abs().max() / ys["off"].abs().max())
            dy = torch.randn(ys["off"].shape, device=dev, generator=gen).to(dt)
            del ys
            line = json.dumps(dict(head, layer=layer, format=fmt,
                                   workload="DAUConv1d N=%d C=256->256 HW=56 G=4 k=%d mu1~U(-%g,%g) fwd+bwd" % (N, k, m, m),
                                   gather_dense_split={n: nets[n]._line_info for n in nets},
                                   max_abs_y_diff_over_max_norm=float("%.3e" % err), **measure(nets, x, dy)))
            print(line, flush=True)
            if args.out:
                with open(args.out, "a") as f:
                    f.write(line + "\n")
            del x, dy, nets
            dc._PLANS.clear()
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
