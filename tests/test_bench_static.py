"""CPU: static checks of bench.py / __graft_entry__.py (they only run on the GPU box, so a slip there is not seen by the CPU suite
otherwise).  A function-level `import x` of a module that is imported at the top as well makes `x` a local of the whole function:
every use before that line raises UnboundLocalError -- on the paths the import was not written for."""
import ast
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _shadowing_imports(path):
    tree = ast.parse(open(path).read())
    top = set()
    for node in tree.body:
        if isinstance(node, ast.Import):
            top.update(a.asname or a.name.split(".")[0] for a in node.names)
        elif isinstance(node, ast.ImportFrom):
            top.update(a.asname or a.name for a in node.names)
    bad = []
    for fn in ast.walk(tree):
        if isinstance(fn, (ast.FunctionDef, ast.AsyncFunctionDef)):
            for n in ast.walk(fn):
                if isinstance(n, ast.Import):
                    bad += [(fn.name, a.asname or a.name.split(".")[0]) for a in n.names if (a.asname or a.name.split(".")[0]) in top]
                elif isinstance(n, ast.ImportFrom):
                    bad += [(fn.name, a.asname or a.name) for a in n.names if (a.asname or a.name) in top]
    return bad


def test_no_function_shadows_a_module_level_import():
    for f in ("bench.py", "__graft_entry__.py"):
        assert _shadowing_imports(os.path.join(ROOT, f)) == [], f


def test_bench_compiles_and_its_argument_parser_builds():
    src = open(os.path.join(ROOT, "bench.py")).read()
    compile(src, "bench.py", "exec")


def _bench(monkeypatch, argv):
    import importlib
    import sys
    monkeypatch.syspath_prepend(ROOT)
    monkeypatch.setattr(sys, "argv", ["bench.py"] + argv)
    bench = importlib.import_module("bench")
    return bench, bench.parse_args()


def test_plain_run_does_only_the_timed_steps_and_full_restores_the_extras(monkeypatch):
    _, a = _bench(monkeypatch, ["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert (a.full, a.steps, a.warmup, a.check, a.check_params, a.steady_seconds) == (False, 7, 2, 0, 0, 0.0)
    _, a = _bench(monkeypatch, ["--full"])
    assert (a.full, a.check, a.check_params, a.steady_seconds) == (True, 1, 4, 8.0)
    _, a = _bench(monkeypatch, ["--full", "--no-check", "--steady-seconds", "0"])
    assert (a.check, a.check_params, a.steady_seconds) == (0, 0, 0.0)
    _, a = _bench(monkeypatch, ["--check", "2"])           # an explicit gate runs without --full as well
    assert (a.check, a.check_params) == (2, 4)


def test_dump_outputs_writes_float32_and_samples_large_outputs_the_same_way(monkeypatch, tmp_path):
    import numpy as np
    import torch
    bench, _ = _bench(monkeypatch, [])
    big = torch.arange(bench.DUMP_SAMPLE + 5000, dtype=torch.float32).reshape(-1, 8)
    small = torch.randn(1, 3, 2, 4)
    outs = (big.to(torch.bfloat16), big, small, small * 2, small * 3, None)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), outs)
    names = sorted(p.name for p in (tmp_path / "a").iterdir())
    assert names == ["dmu1.npy", "dmu2.npy", "dw.npy", "dx.npy", "y.npy"]          # no file for a gradient the step did not take
    total = 0
    for n in names:
        a, b = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        assert a.dtype == np.float32 and np.array_equal(a, b)
        total += (tmp_path / "a" / n).stat().st_size
    dx = np.load(tmp_path / "a" / "dx.npy")
    assert dx.shape == (bench.DUMP_SAMPLE,) and np.all(np.diff(dx) > 0)             # a sample of distinct elements, in flat order
    assert np.array_equal(np.load(tmp_path / "a" / "dw.npy"), small.numpy())        # small outputs whole, in their shape
    assert 6 * bench.DUMP_SAMPLE * 4 < 64e6 and total < 64e6
