#!/usr/bin/env python3
"""tools/ab_step_libs.py --parent-lib <library of the parent commit> --out FILE: A/B of the north-star step (bench.py) between
another build of the library and this tree's, interleaved rounds of fresh processes on one box, then one rocprofv3 --kernel-trace
--stats run of each build for the per-pass times of the two-limb gather-sum's kernels.  One JSON line per run, a verdict line (this
build's median against the parent's median plus the parent's own min-max spread), one line of kernel times per build.
--lib TAG=PATH adds further builds to the rounds (e.g. bf16_e2=.../libdau_conv_hip_bf16_e2.so), --bench-args the workload
(e.g. "--io bf16 --no-check", "--workload c2 --io bf16"), --kernels the kernel-name parts the rocprofv3 line keeps,
--no-prof leaves the rocprofv3 runs out.  The verdict line then also carries, per profile slot (roofline.kernels of bench.py:
gather_dot, ...), every build's values, median and max - min over the rounds.
--fused-layer FORMAT (fp32, f16, bf16) times, instead of bench.py, the layer step with the bias and the ReLU fused into the store
(tools/fused_epilogue_step_time.py, its `fused` leg, one round of --steps per process): the epilogue kernels of the two builds."""
import argparse, csv, glob, json, os, statistics, subprocess, sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--parent-lib", required=True)
ap.add_argument("--out", required=True, help="JSON-lines file to write; the rocprofv3 scratch directories go next to it")
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--steps", type=int, default=40)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--lib", action="append", default=[], metavar="TAG=PATH", help="a further build to interleave (repeatable)")
ap.add_argument("--bench-args", default="", help="further bench.py arguments, one string")
ap.add_argument("--kernels", default="split_absmax,split_scales,split_stage,split_densify,split_gather_kernel",
                help="comma-separated parts of the kernel names kept from the rocprofv3 statistics")
ap.add_argument("--no-prof", action="store_true")
ap.add_argument("--fused-layer", default=None, metavar="FORMAT", help="time the fused bias + ReLU layer step in this format instead of bench.py")
args = ap.parse_args()
OUT = os.path.dirname(os.path.abspath(args.out))
LIBS = [("parent", os.path.abspath(args.parent_lib))] + [(t.split("=", 1)[0], os.path.abspath(t.split("=", 1)[1])) for t in args.lib] + \
       [("this", os.path.join(ROOT, "dau-convnet_amd", "dau_conv", "libdau_conv_hip.so"))]
ROUNDS, STEPS, WARMUP = args.rounds, args.steps, args.warmup
BENCH = [sys.executable, "bench.py", "--gpus", "1", "--steps", str(STEPS), "--warmup", str(WARMUP)] + args.bench_args.split()
if args.fused_layer:
    BENCH = [sys.executable, os.path.join("tools", "fused_epilogue_step_time.py"), "--formats", args.fused_layer, "--rounds", "1",
             "--steps", str(STEPS), "--warmup", str(WARMUP)]
KEEP = tuple(k for k in args.kernels.split(",") if k)
os.makedirs(OUT, exist_ok=True)
lines = open(args.out, "w")


def emit(d):
    lines.write(json.dumps(d) + "\n"); lines.flush()
    print(json.dumps(d)[:600], flush=True)


def run(cmd, env, limit):
    p = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd, cwd=ROOT, env=env, capture_output=True, text=True)
    if p.returncode != 0:
        print("rc", p.returncode, "of", cmd, "\n", p.stdout[-1500:], p.stderr[-3000:], flush=True)
        sys.exit(p.returncode)           # nothing more on the GPU after a failure
    return p.stdout


ms = {t: [] for t, _ in LIBS}
slots = {t: {} for t, _ in LIBS}
for rnd in range(ROUNDS):
    for tag, lib in LIBS:
        env = dict(os.environ, DAU_CONV_LIB=lib)
        d = json.loads([l for l in run(BENCH, env, 280).splitlines() if l.startswith("{")][-1])
        if args.fused_layer:
            ms[tag].append(d["median_ms"]["fused"])
            emit(dict(call="fused_epilogue_step_time", round=rnd, build=tag, ms_per_step=d["median_ms"]["fused"], format=args.fused_layer,
                      steps=STEPS, warmup=WARMUP, build_id=d.get("build_id"), workload=d["workload"]))
            continue
        ms[tag].append(d["ms_per_step"])
        for k, v in ((d.get("roofline") or {}).get("kernels") or {}).items():
            slots[tag].setdefault(k, []).append(v.get("avg_ms"))
        emit(dict(call="bench", round=rnd, build=tag, ms_per_step=d["ms_per_step"], value=d["value"], unit=d["unit"], steps=STEPS, warmup=WARMUP,
                  lib=d.get("lib"), parity_gate=d.get("parity_gate"),
                  kernels_avg_ms={k: v.get("avg_ms") for k, v in (d.get("roofline") or {}).get("kernels", {}).items()},
                  workload=d["config"]["workload"]))
med = {t: statistics.median(v) for t, v in ms.items()}
spread = max(ms["parent"]) - min(ms["parent"])
emit(dict(call="verdict", rounds=ROUNDS, ms_per_step=ms, median_ms=med, parent_min_max_spread_ms=round(spread, 4),
          this_minus_parent_median_ms=round(med["this"] - med["parent"], 4), within_parent_spread=bool(med["this"] <= med["parent"] + spread),
          slots_avg_ms={t: {k: dict(values=v, median=statistics.median(v), max_minus_min=round(max(v) - min(v), 4)) for k, v in sl.items()}
                        for t, sl in slots.items()}, bench_args=args.bench_args, fused_layer=args.fused_layer))

for tag, lib in ([] if args.no_prof else LIBS):
    d = os.path.join(OUT, "prof_" + tag)
    env = dict(os.environ, DAU_CONV_LIB=lib)
    run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "x", "--"] + BENCH, env, 400)
    stats = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
    rows = {}
    for r in csv.DictReader(open(stats[0])):
        name = r["Name"]
        if any(k in name for k in KEEP):
            key = name.replace("(anonymous namespace)::", "").split("(")[0][:90]
            rows[key] = dict(calls=int(r["Calls"]), avg_us=round(float(r["AverageNs"]) / 1e3, 2), total_ms=round(float(r["TotalDurationNs"]) / 1e6, 3))
    emit(dict(call="rocprofv3 --kernel-trace --stats", build=tag, steps=STEPS, warmup=WARMUP, kernels=rows))
    subprocess.run(["rm", "-rf", d])
