"""A/B of the radius-3 + ring gather-sum member (DAU_FLAG_DENSE_SPLIT_OUTLIERS) at the north-star layer: N=128 C=256->256 56x56,
G=4, max_kernel_size 9, sigma 0.5, forward + backward through the plan API.  Offsets: mu ~ U(-3, 3) with a fraction P of the units
redrawn into +-(3, 3.99] on one axis or both, and mu ~ U(-3.99, 3.99) ("uniform": 43 % of the units beyond +-3, the call falls back).

Three configurations per P, each round of each in a FRESH child process, the rounds interleaved (off, on, parent, off, on, ...):
  off     this build, flag off            on      this build, flag on            parent  another library of the same ABI, flag off
                                                                                          (--parent-lib, loaded through DAU_CONV_LIB)
Every child runs under its own `timeout -k 10`; the first child that fails, is killed or times out ends the run (nothing more is
started on the device).  Per (P, configuration): the two gather-sum profile slots (ms per pass: for the ring member the slot
brackets the ring pass and the GEMM), their sum, and the whole forward + backward step (HIP events), medians over the rounds; the
spread of the parent's rounds; which path ran (dau_conv_gather_outlier_status).  One JSON line at the end (--out FILE also writes it).

  python tools/ab_dense_outliers.py --parent-lib /path/to/parent/libdau_conv_hip.so [--rounds 3] [--steps 8] [--warmup 3]
      [--fractions 0,0.001,0.01,0.1,uniform] [--on-lib LIB --limit-permille 1000]
--on-lib / --limit-permille: run `on` on the tuning build with the count limit set (DAU_RING_LIMIT_PERMILLE), for the sweep that
determines the limit: the member must run at every P it is timed at."""
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

NS = dict(N=128, S=256, F=256, H=56, W=56, G=4, k=9)


def child(args):
    import torch
    from dau_conv import _capi
    N, S, F, H, W, G, k = (NS[q] for q in ("N", "S", "F", "H", "W", "G", "k"))
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev)
    gen.manual_seed(1234)
    x = torch.rand((N, S, H, W), device=dev, generator=gen)
    dy = torch.randn((N, F, H, W), device=dev, generator=gen)
    w = torch.randn((1, S, G, F), device=dev, generator=gen) * 0.1
    sigma = torch.full((1, S, G, F), 0.5, device=dev)
    flags = _capi.FLAG_USE_INTERPOLATION | (_capi.FLAG_DENSE_SPLIT_OUTLIERS if args.child == "on" else 0)
    plan = _capi.Plan(N, S, F, G, H, W, max_kernel_size=k, flags=flags, sigma_hint=0.5, mu_learning_rate_factor=1.0)
    rnd = lambda: torch.rand((1, S, G, F), device=dev, generator=gen)
    out = {"config": args.child, "build_id": _capi.build_id(), "device": torch.cuda.get_device_name(0),
           "gather_dense_split": plan.info["gather_dense_split"], "results": {}}
    for frac in args.fractions.split(","):
        if frac == "uniform":
            mu1, mu2 = (rnd() * 2 - 1) * 3.99, (rnd() * 2 - 1) * 3.99
        else:
            mu1, mu2 = (rnd() * 2 - 1) * 3.0, (rnd() * 2 - 1) * 3.0
            pick, axis = rnd() < float(frac), rnd()
            far = lambda: (3.0 + 0.99 * rnd()) * torch.where(rnd() < 0.5, -1.0, 1.0)
            mu1 = torch.where(pick & (axis < 2 / 3), far(), mu1)
            mu2 = torch.where(pick & (axis > 1 / 3), far(), mu2)
        mu1, mu2 = mu1.clamp(-3.99, 3.99).contiguous(), mu2.clamp(-3.99, 3.99).contiguous()
        beyond = int((torch.maximum(mu1.abs(), mu2.abs()) > 3).sum())

        def step():
            plan.forward(x, w, mu1, mu2, sigma)
            plan.backward(x, dy, w, mu1, mu2, sigma)
        for _ in range(args.warmup):
            step()
        torch.cuda.synchronize()
        plan.profile_begin()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.steps):
            step()
        b.record()
        torch.cuda.synchronize()
        prof = plan.profile_end()
        plan.check_status()
        res = {"units_beyond_3": beyond, "step_ms": round(a.elapsed_time(b) / args.steps, 4)}
        for slot in ("gather_sum_fwd", "gather_sum_dx"):
            ms, passes = prof[slot]
            res[slot + "_ms"] = round(ms / max(passes, 1), 4)
        res["gather_sum_ms"] = round(res["gather_sum_fwd_ms"] + res["gather_sum_dx_ms"], 4)
        if hasattr(_capi.lib, "dau_conv_gather_outlier_status"):
            units, taken = plan.outlier_status()
            res["outlier_units"], res["ring_taken"] = units, taken
        out["results"][frac] = res
    print("AB_CHILD " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None, help="library of the commit to compare against (flag off)")
    ap.add_argument("--on-lib", default=None, help="library for the `on` configuration (default: this build's release library)")
    ap.add_argument("--limit-permille", type=int, default=None, help="DAU_RING_LIMIT_PERMILLE for `on` (tuning build only)")
    ap.add_argument("--fractions", default="0,0.001,0.01,0.1,uniform")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=150, help="seconds per child process")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", choices=("off", "on", "parent"), default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)

    configs = ["off", "on"] + (["parent"] if args.parent_lib else [])
    rounds = {c: [] for c in configs}
    for r in range(args.rounds):
        for c in configs:
            env = dict(os.environ)
            env.pop("DAU_CONV_LIB", None)
            env.pop("DAU_RING_LIMIT_PERMILLE", None)
            if c == "parent":
                env["DAU_CONV_LIB"] = os.path.abspath(args.parent_lib)
            if c == "on" and args.on_lib:
                env["DAU_CONV_LIB"] = os.path.abspath(args.on_lib)
            if c == "on" and args.limit_permille is not None:
                env["DAU_RING_LIMIT_PERMILLE"] = str(args.limit_permille)
            cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--child", c,
                   "--fractions", args.fractions, "--steps", str(args.steps), "--warmup", str(args.warmup)]
            done = subprocess.run(cmd, env=env, capture_output=True, text=True)
            line = [l for l in done.stdout.splitlines() if l.startswith("AB_CHILD ")]
            if done.returncode != 0 or not line:
                # a child that failed ends the run: nothing more is started on the device
                sys.stderr.write(done.stdout[-2000:] + done.stderr[-4000:])
                sys.exit("round %d, configuration %s: exit status %d -- run ended" % (r, c, done.returncode))
            rounds[c].append(json.loads(line[0][len("AB_CHILD "):]))
            print("round %d %-6s %s" % (r, c, json.dumps(rounds[c][-1]["results"])), flush=True)

    keys = ("gather_sum_fwd_ms", "gather_sum_dx_ms", "gather_sum_ms", "step_ms")
    summary = {"workload": "ns N=128 C=256->256 HW=56 G=4 k=9 fwd+bwd; mu~U(-3,3), fraction P of units redrawn into +-(3,3.99]",
               "device": rounds["off"][0]["device"], "rounds": args.rounds, "steps_per_round": args.steps,
               "build_id": {c: rounds[c][0]["build_id"] for c in configs}, "limit_permille": args.limit_permille, "fractions": {}}
    for frac in args.fractions.split(","):
        row = {}
        for c in configs:
            rs = [r["results"][frac] for r in rounds[c]]
            row[c] = {k: round(statistics.median(x[k] for x in rs), 4) for k in keys}
            row[c]["spread_ms"] = {k: round(max(x[k] for x in rs) - min(x[k] for x in rs), 4) for k in ("gather_sum_ms", "step_ms")}
            row[c]["rounds_gather_sum_ms"] = [x["gather_sum_ms"] for x in rs]
            row[c]["ring_taken"] = rs[0].get("ring_taken")
            row["units_beyond_3"] = rs[0]["units_beyond_3"]
        if "parent" in row:
            for c in ("off", "on"):
                row[c + "_over_parent"] = {k: round(row[c][k] / row["parent"][k], 4) for k in ("gather_sum_ms", "step_ms")}
        summary["fractions"][frac] = row
    print("%-8s %9s | %s" % ("P", "units>3", " | ".join("%-6s fwd    dx   sum   step" % c for c in configs)))
    for frac, row in summary["fractions"].items():
        print("%-8s %9d | %s" % (frac, row["units_beyond_3"], " | ".join(
            "%-6s %5.2f %5.2f %5.2f %6.2f" % (("ring" if row[c]["ring_taken"] else ""), row[c]["gather_sum_fwd_ms"], row[c]["gather_sum_dx_ms"],
                                              row[c]["gather_sum_ms"], row[c]["step_ms"]) for c in configs)))
    text = json.dumps(summary)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
